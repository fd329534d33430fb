"""porousfreezethaw_amd -- MI355X-native RK-Merson solver + intertrack freezing model.

The product is the C library ``lib/libpft.so`` (host C + HIP kernels for gfx950); this module is
a thin ctypes view of its C ABI for tests, the benchmark and scripting.  Names and argument
meaning follow the reference's C interface (include/RK_MPI_SAsolver.h, equation.c, model.c).
There is no CPU fallback: if the library (or a GPU, for the solving calls) is missing, the calls
fail loudly.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB_PATH = os.environ.get("PFT_LIB") or os.path.join(HERE, "lib", "libpft.so")

PARAM_NAMES = [  # model.c:44-59, the order of param[] (include/pft_model.h)
    "u_star", "L", "xi", "a", "b", "alpha", "mu",
    "beads_scaling", "beads_offset_x", "beads_offset_y", "beads_offset_z",
    "xi_gl", "zeta", "p_eps0", "p_eps1", "gamma",
    "water_cp", "ice_cp", "glass_cp", "water_lambda", "ice_lambda", "glass_lambda",
    "water_rho", "ice_rho", "glass_rho", "top_temp1", "top_temp2", "phase_switch_time",
    "u_noise_amp", "ball_radius",
]
BCOND_THICKNESS = 2
DELTA_LOCAL, DELTA_GLOBAL = 0, 1
RKA_CMD_FINISHED = 8
PFT_SOLVE_KEEP_DEVICE, PFT_SOLVE_REUSE_DEVICE = 1, 2
PFT_OPT_GL_STATIC, PFT_OPT_KZ, PFT_OPT_DEVICE, PFT_OPT_TIMING, PFT_OPT_TILE, PFT_OPT_RECOMPUTE = 1, 2, 3, 4, 5, 6
PFT_OPT_LAZY_ALLOC = 9
PFT_OPT_PAIR = 10
PFT_OPT_GATE = 12
PFT_OPT_FAIL_RHS = 11
PFT_SOLVE_DEVICE_ERROR = -7
PFT_SNAP_ASYNC, PFT_SNAP_DIRECT, PFT_SNAP_STAGED = 1, 2, 4      # include/pft_solver.h
PFT_BUF_X, PFT_BUF_XN = 0, 1                                     # include/pft_hip.h
MPI_COMM_WORLD = 0x44000000

# every function of the public headers, for the "library exports its ABI" check
ABI_FUNCTIONS = [
    "RK_MPI_SA_init", "RK_MPI_SA_cleanup", "RK_MPI_SA_handle_NAN", "RK_MPI_SA_check_NAN",
    "RK_MPI_SA_check_mem", "RK_MPI_SA_solve",
]


class RK_MEM_DIST(C.Structure):
    _fields_ = [("n_chunks", C.c_int), ("chunk_start", C.POINTER(C.c_int)),
                ("chunk_size", C.POINTER(C.c_int)), ("chunk_eps_mult", C.POINTER(C.c_double))]


RHS_FN = C.CFUNCTYPE(None, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double))
META_FN = C.CFUNCTYPE(C.c_void_p)


class RK_MPI_S_SOLUTION(C.Structure):
    pass


SERVICE_FN = C.CFUNCTYPE(C.c_int, C.c_double, C.POINTER(RK_MPI_S_SOLUTION))
REARRANGE_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p)   # RK_MEM_DIST* (*)(RK_MEM_DIST*)
RK_MPI_S_SOLUTION._fields_ = [
    ("n", C.POINTER(RK_MEM_DIST)), ("t", C.c_double), ("x", C.POINTER(C.c_double)),
    ("meta_f", C.c_void_p), ("h", C.c_double), ("h_min", C.c_double), ("delta", C.c_double),
    ("delta_mode", C.c_int), ("DDLBF_Rearrange", C.c_void_p), ("Service_Callback", C.c_void_p),
    ("steps", C.c_long), ("steps_total", C.c_long)]


class pft_grid(C.Structure):
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("n3", C.c_int), ("total_n3", C.c_int),
                ("first_row", C.c_int), ("rank", C.c_int), ("nprocs", C.c_int),
                ("L1", C.c_double), ("L2", C.c_double), ("L3", C.c_double), ("calc_mode", C.c_int)]


class pft_snapshot_info(C.Structure):
    """include/pft_io.h: the attributes of a snapshot dataset (intertrack.c:2393-2406)"""
    _fields_ = [("t", C.c_double), ("tau", C.c_double), ("final_time", C.c_double), ("delta", C.c_double),
                ("snapshot", C.c_int), ("total_snapshots", C.c_int), ("calc_mode", C.c_int),
                ("title", C.c_char * 256), ("L1", C.c_double), ("L2", C.c_double), ("L3", C.c_double)]


class pft_snapshot_ranges(C.Structure):
    """include/pft_io.h: where a slab's image lies in a dataset"""
    _fields_ = [("off", C.c_ulonglong * 3), ("bytes", C.c_ulonglong)]


class pft_region(C.Structure):
    """include/pft_io.h: per axis start, count, stride in global interior indices; [0] = i, [1] = j, [2] = k"""
    _fields_ = [("start", C.c_int * 3), ("count", C.c_int * 3), ("stride", C.c_int * 3)]

    def selection(self):
        """the numpy index of the region in a [k, j, i] array: three slices"""
        return tuple(slice(self.start[a], self.start[a] + (self.count[a] - 1) * self.stride[a] + 1, self.stride[a])
                     for a in (2, 1, 0))


class pft_solver_stats(C.Structure):
    _fields_ = [("path", C.c_int), ("nprocs", C.c_int), ("rank", C.c_int),
                ("kernel_launches", C.c_long), ("steps_total", C.c_long), ("last_eps", C.c_double),
                ("stage_ms", C.c_double * 6), ("stage_n", C.c_long * 6), ("pairs", C.c_int),
                ("gated_steps", C.c_long), ("gate_misses", C.c_long)]


class pft_diag_opts(C.Structure):
    """include/pft_diag.h: the thresholds (the published scripts': 0.5, 0.5)"""
    _fields_ = [("p_thr", C.c_double), ("gl_thr", C.c_double)]


class pft_diag(C.Structure):
    """include/pft_diag.h: the ice diagnostics of a state -- counts and maxima, exact"""
    _fields_ = [("cells", C.c_longlong), ("ice", C.c_longlong), ("pore", C.c_longlong),
                ("ice_pore", C.c_longlong), ("nonfinite", C.c_longlong), ("ice_u_maxabs", C.c_double),
                ("u_min", C.c_double), ("u_max", C.c_double), ("p_min", C.c_double), ("p_max", C.c_double)]

    def as_dict(self):
        """the fields and ice_fraction = ice / cells (correctly rounded: what ncwa gets from an
        exact sum of 0/1 values)"""
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["ice_fraction"] = d["ice"] / d["cells"] if d["cells"] else float("nan")
        return d


PFT_XSUM_WORDS = 66
MEAN_KEYS = ("u", "p", "ice_u", "pore_p")     # include/pft_means.h: PFT_MEAN_U, _P, _U_ICE, _P_PORE


class pft_xsum(C.Structure):
    """include/pft_means.h: value = sum_j w[j] * 2^(32 j - 1074), exactly"""
    _fields_ = [("w", C.c_longlong * PFT_XSUM_WORDS)]

    def as_int(self):
        """the exact sum in units of 2^-1074, a Python integer"""
        return sum(int(w) << (32 * j) for j, w in enumerate(self.w))


class pft_means(C.Structure):
    """include/pft_means.h: per quantity the count of the cells that entered and their exact sum"""
    _fields_ = [("n", C.c_longlong * len(MEAN_KEYS)), ("sum", pft_xsum * len(MEAN_KEYS))]

    def words(self):
        """the raw words, counts first: equal lists <=> equal records"""
        return list(self.n) + [int(w) for s in self.sum for w in s.w]

    def values(self, q):
        """(n, correctly rounded sum, correctly rounded mean) of quantity q; the mean is the exact
        quotient sum / n rounded once (CPython's integer true division is correctly rounded), NaN
        when no cell entered"""
        n, total = int(self.n[q]), self.sum[q].as_int()
        out = C.c_double()
        rc = lib().pft_xsum_round(C.byref(self.sum[q]), C.byref(out))
        if rc:
            raise RuntimeError(f"pft_xsum_round failed ({rc})")
        if n == 0:
            return 0, out.value, float("nan")
        try:
            mean = total / (n << 1074)
        except OverflowError:     # past DBL_MAX: only a sum that itself rounds to +-Inf can
            mean = float("inf") if total > 0 else float("-inf")
        return n, out.value, mean

    def as_dict(self):
        d = {}
        for q, k in enumerate(MEAN_KEYS):
            d[k + "_n"], d[k + "_sum"], d[k + "_mean"] = self.values(q)
        return d


PFT_FORMULA_MAX, PFT_FORMULA_MAX_ENTRIES = 8, 256     # include/pft_formula.h
FORMULA_INPUTS = ("x", "y", "z", "_x", "_y", "_z", "u", "p", "gl")    # inputs 0..8 of a program (pft_frontend.h)
FORMULA_ROW_KEYS = ("mean", "sum", "n", "nonzero", "min", "max", "maxabs")   # run_series: <name>_<key>


class pft_fdiag(C.Structure):
    """include/pft_formula.h: the record of one formula over the interior cells -- counts, ordered
    extrema and the exact sum"""
    _fields_ = [("cells", C.c_longlong), ("n", C.c_longlong), ("nonzero", C.c_longlong),
                ("nonfinite", C.c_longlong), ("min", C.c_double), ("max", C.c_double), ("maxabs", C.c_double),
                ("sum", pft_xsum)]

    def words(self):
        """the raw words, counts first, the doubles as their bits: equal lists <=> equal records"""
        bits = np.array([self.min, self.max, self.maxabs], dtype=np.float64).view(np.uint64)
        return ([int(self.cells), int(self.n), int(self.nonzero), int(self.nonfinite)] + [int(b) for b in bits]
                + [int(w) for w in self.sum.w])

    def as_dict(self):
        """cells, n, nonzero, nonfinite, min, max, maxabs, sum (the exact sum rounded once) and mean
        (the exact quotient sum / n rounded once, NaN when n is 0), as pft_means.values"""
        d = {k: getattr(self, k) for k in ("cells", "n", "nonzero", "nonfinite", "min", "max", "maxabs")}
        out = C.c_double()
        rc = lib().pft_xsum_round(C.byref(self.sum), C.byref(out))
        if rc:
            raise RuntimeError(f"pft_xsum_round failed ({rc})")
        d["sum"] = out.value
        n, total = int(self.n), self.sum.as_int()
        if n == 0:
            d["mean"] = float("nan")
        else:
            try:
                d["mean"] = total / (n << 1074)
            except OverflowError:
                d["mean"] = float("inf") if total > 0 else float("-inf")
        return d


def formula_programs(formulas, variables=None):
    """{name: expression} -> (names, lens, ops, args): the postfix programs of frontend.Evaluator.compile,
    concatenated for pft_formula_host / pft_solver_formulas.  variables: a {name: value} dict or a
    frontend.Evaluator whose variables the expressions may use (it is not changed).  The nine node
    inputs x, y, z, _x, _y, _z, u, p, gl always mean the node's own values, whatever `variables`
    defines -- the rule of Case.icond_programs.  ValueError (frontend.EvalError is one) for an empty
    dict, more than PFT_FORMULA_MAX formulas, an undefined symbol, a syntax error or more than
    PFT_FORMULA_MAX_ENTRIES program entries in all."""
    from .frontend import VAR, EvalError, Evaluator
    if not isinstance(formulas, dict) or not formulas:
        raise ValueError("formulas: a non-empty {name: expression} dict")
    if len(formulas) > PFT_FORMULA_MAX:
        raise ValueError(f"formulas: at most {PFT_FORMULA_MAX} per call, not {len(formulas)}")
    ev = Evaluator()
    if isinstance(variables, Evaluator):
        for name, kind, _, value, _ in variables.ident:
            if kind == VAR:
                ev.define(name, value)
    elif variables is not None:
        for name, value in dict(variables).items():
            ev.define(str(name), float(value))
    for v in FORMULA_INPUTS:
        ev.define(v, 0.5)
    names, progs = [], []
    for name, expr in formulas.items():
        try:
            prog = ev.compile(str(expr), FORMULA_INPUTS, evaluate=False)
        except EvalError as e:
            raise EvalError(f"formula {name!r} ({expr!r}): {e}") from None
        names.append(str(name))
        progs.append(prog)
    if sum(len(pr) for pr in progs) > PFT_FORMULA_MAX_ENTRIES:
        raise ValueError(f"formulas: the programs have {sum(len(pr) for pr in progs)} entries, more than "
                         f"{PFT_FORMULA_MAX_ENTRIES}")
    lens = np.array([len(pr) for pr in progs], dtype=np.int32)
    ops = np.array([o for pr in progs for o, _ in pr], dtype=np.int32)
    args = np.array([a for pr in progs for _, a in pr], dtype=np.float64)
    return names, lens, ops, args


PFT_HIST_MAX_BINS = 1024                               # include/pft_hist.h
HIST_ROW_KEYS = ("under", "over", "nan", "selected")   # run_series: <name> (the counts) and <name>_<key>


class pft_hist_head(C.Structure):
    """include/pft_hist.h: the head of a histogram record; selected == nan + under + over + sum(counts)"""
    _fields_ = [("cells", C.c_longlong), ("selected", C.c_longlong), ("nan", C.c_longlong),
                ("under", C.c_longlong), ("over", C.c_longlong)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class pft_hist_prog(C.Structure):
    """include/pft_hist.h: a formula as pft_hist_host takes it"""
    _fields_ = [("n", C.c_int), ("op", C.POINTER(C.c_int)), ("arg", C.POINTER(C.c_double))]


def hist_edges(bins, range=None):
    """The edge array of a histogram (f13), float64 [nbins + 1] -- the contract of every histogram
    entry, which returns it too.  An int `bins` with range=(lo, hi): np.linspace(lo, hi, bins + 1);
    an array is taken as the edges (range must then be None).  ValueError for everything
    pft_hist_check refuses: fewer than 1 or more than PFT_HIST_MAX_BINS bins, an edge that is NaN
    or +-Inf, edges that are not strictly increasing (equal neighbours, -0.0 next to +0.0)."""
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        if range is None:
            raise ValueError("hist_edges: an int `bins` needs range=(lo, hi)")
        if not 1 <= int(bins) <= PFT_HIST_MAX_BINS:
            raise ValueError(f"hist_edges: bins must be in 1..{PFT_HIST_MAX_BINS}, not {bins}")
        try:
            lo, hi = (float(v) for v in range)
        except (TypeError, ValueError):
            raise ValueError(f"hist_edges: range must be (lo, hi), not {range!r}") from None
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError(f"hist_edges: range must be finite with lo < hi, not {range!r}")
        edges = np.linspace(lo, hi, int(bins) + 1)
    else:
        if range is not None:
            raise ValueError("hist_edges: range= goes with an int `bins`, not with an edge array")
        try:
            edges = np.ascontiguousarray(bins, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"hist_edges: bins must be an int or an array of edges, not {bins!r}") from None
        if edges.ndim != 1 or not 2 <= edges.size <= PFT_HIST_MAX_BINS + 1:
            raise ValueError(f"hist_edges: 2..{PFT_HIST_MAX_BINS + 1} edges in one dimension, not shape {edges.shape}")
        edges = edges.copy()
    if lib().pft_hist_check(edges.size - 1, _dp(edges)):
        raise ValueError("hist_edges: the edges must be finite and strictly increasing")
    return edges


def hist_spec(formula, bins, range=None, mask=None, variables=None):
    """A histogram compiled for Simulation.histogram / run_series: the edges (hist_edges) and the
    postfix programs of the value formula and of the optional mask formula (formula_programs; its
    `variables`).  ValueError before any work for bad edges, an undefined symbol or a syntax error."""
    edges = hist_edges(bins, range)
    value = formula_programs({"formula": formula}, variables)
    masked = None if mask is None else formula_programs({"mask": mask}, variables)
    if masked is not None and len(value[2]) + len(masked[2]) > PFT_FORMULA_MAX_ENTRIES:
        raise ValueError(f"histogram: formula and mask together have more than {PFT_FORMULA_MAX_ENTRIES} entries")
    return {"compiled": True, "formula": str(formula), "mask": None if mask is None else str(mask), "edges": edges,
            "value": value, "masked": masked}


def hist_quantile(h, q):
    """The bracket (lo, hi) of the bin that holds the q-quantile (0 <= q <= 1) of the selected values
    that are not NaN, of a histogram dict `h` (edges, counts, under, over): the first bin, in the
    order under, the bins, over, at which the cumulated count reaches ceil(q * N), at least 1.
    (-inf, edges[0]) or (edges[-1], inf) when it falls in under or over.  Integer arithmetic only:
    q enters as the exact ratio of the double.  ValueError for a q outside [0, 1] or when N is 0."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"hist_quantile: q must be in [0, 1], not {q!r}")
    edges = h["edges"]
    counts = [int(c) for c in h["counts"]]
    under, over = int(h["under"]), int(h["over"])
    total = under + sum(counts) + over
    if total == 0:
        raise ValueError("hist_quantile: no selected value that is not NaN")
    num, den = q.as_integer_ratio()
    target = max(1, -(-num * total // den))
    cum = under
    if cum >= target:
        return (float("-inf"), float(edges[0]))
    for b, c in enumerate(counts):
        cum += c
        if cum >= target:
            return (float(edges[b]), float(edges[b + 1]))
    return (float(edges[-1]), float("inf"))


def write_hist_txt(rows, path, key):
    """one line per snapshot: the counts of histogram `key` (run_series(histograms=)'s rows) as
    decimal integers separated by blanks"""
    with open(path, "w") as f:
        for r in rows:
            f.write(" ".join(str(int(c)) for c in r[key]) + "\n")


MAP_KEYS = ("selected", "nonzero", "nonfinite", "min", "max", "first", "last")   # include/pft_map.h


class pft_map_px(C.Structure):
    """include/pft_map.h: one pixel of a map (f15), 56 bytes"""
    _fields_ = [("selected", C.c_longlong), ("nonzero", C.c_longlong), ("nonfinite", C.c_longlong),
                ("min", C.c_double), ("max", C.c_double), ("first", C.c_longlong), ("last", C.c_longlong)]


MAP_DTYPE = np.dtype([(k, "<f8" if k in ("min", "max") else "<i8") for k in MAP_KEYS])   # pft_map_px as numpy sees it


def map_spec(formula, axis, mask=None, variables=None):
    """A map compiled for Simulation.project / run_series: the axis (0 z, 1 y, 2 x -- numpy's
    numbering of interior()'s [k, j, i]) and the postfix programs of the value formula and of the
    optional mask formula (formula_programs; its `variables`).  ValueError before any work for an
    axis outside 0..2, an undefined symbol or a syntax error."""
    if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or not 0 <= int(axis) <= 2:
        raise ValueError(f"project: axis must be 0 (z), 1 (y) or 2 (x), not {axis!r}")
    value = formula_programs({"formula": formula}, variables)
    masked = None if mask is None else formula_programs({"mask": mask}, variables)
    if masked is not None and len(value[2]) + len(masked[2]) > PFT_FORMULA_MAX_ENTRIES:
        raise ValueError(f"project: formula and mask together have more than {PFT_FORMULA_MAX_ENTRIES} entries")
    return {"compiled": True, "formula": str(formula), "mask": None if mask is None else str(mask), "axis": int(axis),
            "value": value, "masked": masked}


def _map_ptr(a):
    return a.ctypes.data_as(C.POINTER(pft_map_px))


class pft_ic_prog(C.Structure):
    """include/pft_frontend.h: a program compiled for the device (owned by the library: pft_ic_prog_free)"""
    _fields_ = [("n", C.c_int), ("op", C.POINTER(C.c_int)), ("arg", C.POINTER(C.c_double)), ("ntab", C.c_int),
                ("tab_axis", C.POINTER(C.c_int)), ("tab_off", C.POINTER(C.c_long)),
                ("tab_val", C.POINTER(C.c_double)), ("tab_err", C.POINTER(C.c_ubyte)), ("tab_len", C.c_long),
                ("const_err", C.c_int)]


_lib = None


def lib():
    """Load libpft.so (built in-tree by __graft_entry__.build() / make -C porousfreezethaw_amd)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libpft.so is not built ({LIB_PATH}); run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)   # RTLD_LOCAL: its ROCm 7.2 runtime must not interpose on torch's
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.RK_MPI_SA_init.argtypes = [C.c_int, C.c_int, C.c_int]
        L.RK_MPI_SA_check_mem.argtypes = [C.POINTER(RK_MEM_DIST)]
        L.RK_MPI_SA_solve.argtypes = [C.c_double, C.POINTER(RK_MPI_S_SOLUTION)]
        L.RK_MPI_SA_handle_NAN.argtypes = [C.c_int]
        L.RK_MPI_SA_handle_NAN.restype = None
        L.pft_solve_ex.argtypes = [C.c_double, C.POINTER(RK_MPI_S_SOLUTION), C.c_long, C.c_int]
        L.pft_solver_download.argtypes = [C.POINTER(RK_MPI_S_SOLUTION)]
        L.pft_solver_set_option.argtypes = [C.c_int, C.c_long]
        L.pft_solver_get_stats.argtypes = [C.POINTER(pft_solver_stats)]
        L.pft_solver_last_status.restype = C.c_int
        L.pft_solver_slab.restype = C.c_void_p
        L.pft_slab_tile_geometry.argtypes = [C.c_void_p, C.c_int, ip, ip]
        L.pft_decompose.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip]
        L.pft_decompose.restype = None
        L.pft_grid_init.argtypes = [C.POINTER(pft_grid), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_double, C.c_double, C.c_double, C.c_int]
        L.pft_grid_block.argtypes = [C.POINTER(pft_grid)]
        L.pft_grid_block.restype = C.c_long
        L.pft_model_configure.argtypes = [C.POINTER(pft_grid), dp]
        L.bcond_setup.argtypes = [C.c_double, dp]
        L.bcond_setup.restype = None
        L.pft_model_set_beads.argtypes = [dp, C.c_int]
        L.pft_model_load_beads.argtypes = [C.c_char_p]
        L.PrecalculateData.argtypes = [dp]
        L.pft_model_set_solution.argtypes = [dp]
        L.pft_model_chunks.argtypes = [ip, ip, dp]
        L.pft_model_ic_default.argtypes = [dp]
        L.pft_float_val.argtypes = [C.c_char_p]
        L.pft_float_val.restype = C.c_double
        for name in ("f_generic_model01", "f_generic_model2"):
            getattr(L, name).argtypes = [C.c_double, dp, dp]
            getattr(L, name).restype = None
        for name in ("mf_single", "mf_top", "mf_middle", "mf_bottom"):
            getattr(L, name).restype = C.c_void_p
        L.pft_hip_device_count.argtypes = [ip]
        L.pft_hip_set_device.argtypes = [C.c_int]
        L.pft_ic_device_ok.argtypes = [C.POINTER(pft_grid), C.c_int, ip, dp]
        L.pft_solver_ic_formulas_device.argtypes = [C.c_int, ip, ip, ip, dp, C.c_int]
        L.pft_hip_last_error.restype = C.c_char_p
        L.pft_comm_get_unique_id.argtypes = [C.c_void_p]
        L.pft_comm_init_rccl.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.pft_comm_init_loopback.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.pft_comm_init_ipc.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.pft_comm_device_halo.argtypes = [C.c_void_p]
        L.pft_comm_boundary_first.argtypes = [C.c_void_p]
        L.pft_comm_copy_engine.argtypes = [C.c_void_p]
        L.pft_comm_set_copy_engine.argtypes = [C.c_void_p, C.c_int]
        L.pft_comm_loopback_rank.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.pft_comm_set_current.argtypes = [C.c_void_p]
        L.pft_comm_destroy.argtypes = [C.c_void_p]
        L.pft_comm_set_self_exchange.argtypes = [C.c_void_p, C.c_int]
        L.pft_comm_splits.argtypes = [C.c_void_p]
        L.pft_comm_barrier.argtypes = [C.c_void_p]
        L.pft_comm_current.restype = C.c_void_p
        L.pft_comm_kind.argtypes = [C.c_void_p]
        L.pft_comm_kind.restype = C.c_char_p
        L.pft_slab_stream.argtypes = [C.c_void_p]
        L.pft_slab_stream.restype = C.c_void_p
        L.pft_hip_device_sync.restype = C.c_int
        gp, sp = C.POINTER(pft_grid), C.POINTER(pft_snapshot_info)
        L.pft_ic_eval.argtypes = [gp, C.c_int, C.c_int, ip, dp, dp]
        L.pft_model_noise.restype = dp
        L.pft_snapshot_create.argtypes = [C.c_char_p, gp, dp, sp, C.c_int]
        L.pft_snapshot_write_slab.argtypes = [C.c_char_p, gp, dp]
        L.pft_snapshot_write.argtypes = [C.c_char_p, gp, dp, sp, dp]
        L.pft_snapshot_read_info.argtypes = [C.c_char_p, ip, ip, ip, sp, dp]
        L.pft_snapshot_read_slab.argtypes = [C.c_char_p, gp, dp]
        L.pft_snapshot_title.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_double]
        op, dgp, llp = C.POINTER(pft_diag_opts), C.POINTER(pft_diag), C.POINTER(C.c_longlong)
        L.pft_diag_host.argtypes = [gp, dp, op, dgp, llp]
        L.pft_diag_combine.argtypes = [dgp, dgp]
        L.pft_slab_diag.argtypes = [C.c_void_p, C.c_int, op, dgp, llp]
        L.pft_slab_diag_timing.argtypes = [C.c_void_p, C.c_int]
        L.pft_slab_diag_last_ms.argtypes = [C.c_void_p, dp]
        L.pft_solver_diag.argtypes = [op, dgp, dgp, llp]
        xp, mp = C.POINTER(pft_xsum), C.POINTER(pft_means)
        L.pft_xsum_add.argtypes = [xp, C.c_double]
        L.pft_xsum_combine.argtypes = [xp, xp]
        L.pft_xsum_round.argtypes = [xp, dp]
        L.pft_means_host.argtypes = [gp, dp, op, mp, mp]
        L.pft_means_combine.argtypes = [mp, mp]
        L.pft_slab_means.argtypes = [C.c_void_p, C.c_int, op, mp, mp]
        L.pft_slab_means_timing.argtypes = [C.c_void_p, C.c_int]
        L.pft_slab_means_last_ms.argtypes = [C.c_void_p, dp]
        L.pft_solver_means.argtypes = [op, mp, mp, mp]
        L.pft_comm_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.pft_comm_allgather_any.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        fp, icp = C.POINTER(pft_fdiag), C.POINTER(pft_ic_prog)
        L.pft_fdiag_init.argtypes = [fp]
        L.pft_fdiag_init.restype = None
        L.pft_fdiag_combine.argtypes = [fp, fp]
        L.pft_formula_host.argtypes = [gp, dp, C.c_int, ip, ip, dp, fp, fp]
        L.pft_formula_compile.argtypes = [gp, C.c_int, ip, dp, icp]
        L.pft_ic_prog_free.argtypes = [icp]
        L.pft_ic_prog_free.restype = None
        L.pft_slab_formulas.argtypes = [C.c_void_p, C.c_int, C.c_int, icp, fp, fp]
        L.pft_slab_formulas_timing.argtypes = [C.c_void_p, C.c_int]
        L.pft_slab_formulas_last_ms.argtypes = [C.c_void_p, dp]
        L.pft_solver_formulas.argtypes = [C.c_int, ip, ip, dp, fp, fp, fp]
        hp, hpp, llp = C.POINTER(pft_hist_head), C.POINTER(pft_hist_prog), C.POINTER(C.c_longlong)
        L.pft_hist_check.argtypes = [C.c_int, dp]
        L.pft_hist_bin.argtypes = [C.c_int, dp, C.c_double]
        L.pft_hist_combine.argtypes = [C.c_int, hp, llp, hp, llp]
        L.pft_hist_host.argtypes = [gp, dp, hpp, hpp, C.c_int, dp, hp, llp, hp, llp]
        L.pft_slab_hist.argtypes = [C.c_void_p, C.c_int, icp, icp, C.c_int, dp, hp, llp, hp, llp]
        L.pft_slab_hist_timing.argtypes = [C.c_void_p, C.c_int]
        L.pft_slab_hist_last_ms.argtypes = [C.c_void_p, dp]
        L.pft_solver_hist.argtypes = [C.c_int, ip, dp, C.c_int, ip, dp, C.c_int, dp, hp, llp, hp, llp, hp, llp]
        mp = C.POINTER(pft_map_px)
        L.pft_map_init.argtypes = [mp]
        L.pft_map_init.restype = None
        L.pft_map_combine.argtypes = [C.c_long, mp, mp]
        L.pft_map_dims.argtypes = [gp, C.c_int, ip, ip]
        L.pft_map_host.argtypes = [gp, dp, hpp, hpp, C.c_int, mp]
        L.pft_slab_map.argtypes = [C.c_void_p, C.c_int, icp, icp, C.c_int, mp]
        L.pft_slab_map_timing.argtypes = [C.c_void_p, C.c_int]
        L.pft_slab_map_last_ms.argtypes = [C.c_void_p, dp]
        L.pft_solver_map.argtypes = [C.c_int, ip, dp, C.c_int, ip, dp, C.c_int, mp, mp]
        rp, vpp = C.POINTER(pft_snapshot_ranges), C.POINTER(C.c_void_p)
        L.pft_snapshot_image_bytes.argtypes = [gp]
        L.pft_snapshot_image_bytes.restype = C.c_size_t
        L.pft_snapshot_image_host.argtypes = [gp, dp, C.c_void_p]
        L.pft_snapshot_slab_ranges.argtypes = [C.c_char_p, gp, rp]
        L.pft_snapshot_read_series.argtypes = [C.c_char_p, ip, ip, dp, dp, dp]
        L.pft_snapshot_write_image.argtypes = [C.c_char_p, rp, C.c_void_p]
        L.pft_snapshot_read_image.argtypes = [C.c_char_p, rp, C.c_void_p]
        L.pft_snapshot_write_image_async.argtypes = [C.c_char_p, rp, C.c_void_p]
        L.pft_snapshot_writer_release.argtypes = [C.c_void_p]
        L.pft_slab_image_bytes.argtypes = [C.c_void_p]
        L.pft_slab_image_bytes.restype = C.c_size_t
        L.pft_slab_export_be.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.pft_slab_import_be.argtypes = [C.c_void_p, C.c_void_p, ip]
        L.pft_slab_image.argtypes = [C.c_void_p, vpp, vpp]
        L.pft_slab_snapshot_export.argtypes = [C.c_void_p, C.c_int, C.c_int, vpp]
        L.pft_slab_snapshot_timing.argtypes = [C.c_void_p, C.c_int]
        L.pft_slab_snapshot_last_ms.argtypes = [C.c_void_p, dp]
        L.pft_solver_snapshot_write.argtypes = [C.c_char_p, dp, sp, C.c_int]
        L.pft_solver_snapshot_read.argtypes = [C.c_char_p]
        L.pft_comm_size.argtypes = [C.c_void_p]
        gnp = C.POINTER(pft_region)
        L.pft_region_check.argtypes = [gp, gnp]
        L.pft_region_local.argtypes = [gp, gnp, ip, ip, ip]
        L.pft_region_image_bytes.argtypes = [gp, gnp]
        L.pft_region_image_bytes.restype = C.c_size_t
        L.pft_region_image_host.argtypes = [gp, gnp, dp, C.c_void_p]
        L.pft_snapshot_create_region.argtypes = [C.c_char_p, gp, gnp, dp, sp, C.c_int]
        L.pft_snapshot_region_ranges.argtypes = [C.c_char_p, gp, gnp, rp]
        L.pft_snapshot_write_region.argtypes = [C.c_char_p, gp, gnp, dp, sp, dp, C.c_int]
        L.pft_slab_region_image_bytes.argtypes = [gnp]
        L.pft_slab_region_image_bytes.restype = C.c_size_t
        L.pft_slab_export_region_be.argtypes = [C.c_void_p, C.c_int, gnp, C.c_void_p]
        L.pft_slab_region_export.argtypes = [C.c_void_p, C.c_int, gnp, C.c_int, vpp]
        L.pft_solver_snapshot_region_write.argtypes = [C.c_char_p, dp, sp, gnp, C.c_int]
        L.pft_solver_region.argtypes = [gnp, dp]
        _lib = L
    return _lib


def _dp(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_int))


def device_count():
    n = C.c_int(0)
    rc = lib().pft_hip_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def decompose(total_n3, nprocs, rank):
    n3, fr = C.c_int(), C.c_int()
    lib().pft_decompose(total_n3, nprocs, rank, C.byref(n3), C.byref(fr))
    return n3.value, fr.value


def comm_init_ipc(nranks, rank, name, device=0):
    """the ipc communicator of rank `rank` (pft_comm.h): every rank passes the same shared-memory
    name ("/..."), rank 0 creates it; bound to this thread (pft_comm_set_current).  Returns the handle."""
    c = C.c_void_p()
    rc = lib().pft_comm_init_ipc(C.byref(c), nranks, rank, name.encode(), device)
    if rc:
        raise RuntimeError(f"pft_comm_init_ipc(rank {rank}) failed ({rc}): {lib().pft_hip_last_error()}")
    lib().pft_comm_set_current(c)
    return c


def comm_destroy(c):
    lib().pft_comm_set_current(None)
    lib().pft_comm_destroy(c)


def region(k, j, i, grid):
    """The pft_region (include/pft_io.h) of a selection given the way numpy indexes interior()'s
    [k, j, i] axes on the whole grid: each of k, j, i a slice or an int.  An int n is the single
    index n (negative: from the end), and that axis is kept with length 1.  A slice is normalised
    with slice.indices, as numpy does.  grid: a pft_grid, or (total_n3, n2, n1).  ValueError for a
    step that is not positive, an empty axis and an int past the grid -- before any device work."""
    dims = (grid.total_n3, grid.n2, grid.n1) if isinstance(grid, pft_grid) else tuple(int(v) for v in grid)
    r = pft_region()
    for axis, (name, sel, n) in enumerate(zip("kji", (k, j, i), dims)):
        if isinstance(sel, slice):
            start, stop, step = sel.indices(n)       # (a zero step: slice.indices' own ValueError)
            if step < 1:
                raise ValueError(f"region: the step of {name} must be positive, not {step}")
            count = len(range(start, stop, step))
            if count < 1:
                raise ValueError(f"region: the selection {sel} of {name} is empty on {n} cells")
        else:
            try:
                start = sel.__index__()
            except AttributeError:
                raise ValueError(f"region: {name} must be a slice or an int, not {sel!r}") from None
            if not -n <= start < n:
                raise ValueError(f"region: index {sel} of {name} lies past the grid's {n} cells")
            start, step, count = start % n, 1, 1
        r.start[2 - axis], r.count[2 - axis], r.stride[2 - axis] = start, count, step
    return r


def _check_where(where):
    if where not in ("device", "host"):
        raise ValueError(f"where must be 'device' or 'host', not {where!r}")


def params_array(values):
    """dict name -> value  ->  param[] in model.c order"""
    return np.array([float(values[k]) for k in PARAM_NAMES], dtype=np.float64)


def series_times(t0, final_time, saved_files, first=0):
    """the snapshot times of the driver's loop (intertrack.c:2265-2283) from starting snapshot
    `first` (0, or a continued series': :1650-1662): snapshot `first` is t0 itself, snapshot
    s > first is t0 + ((final_time - t0) * (s - first)) / (saved_files - 1 - first) (:2271), in
    that operation order in double; [t0] alone when first is the last snapshot"""
    t0, final_time, saved_files, first = float(t0), float(final_time), int(saved_files), int(first)
    if saved_files < 1:
        raise ValueError(f"saved_files must be at least 1, not {saved_files}")
    if not 0 <= first < saved_files:
        raise ValueError(f"first must lie in 0 .. {saved_files - 1}, not {first}")
    return [t0] + [t0 + ((final_time - t0) * float(s - first)) / float(saved_files - 1 - first)
                   for s in range(first + 1, saved_files)]


def write_series_txt(rows, path, key="ice_fraction"):
    """one value per line as "%.15g \n" (with the trailing blank): the format of the published
    series files (0.03488 , 0.055108 ); rows: run_series' rows, or any dicts with `key`"""
    with open(path, "w") as f:
        for r in rows:
            f.write("%.15g \n" % r[key])


class Simulation:
    """One slab of an intertrack run, driven exactly like intertrack.c drives the reference.

    Sets up the grid (intertrack.c:1776-1800), the host solution array and chunk table
    (:1803-1827, :2144-2157), the model (equation.c contract), and the solver
    (RK_MPI_SA_init :2192, check_mem :2208, PrecalculateData :2218), then solves with
    RK_MPI_SA_solve (:2283) or the device-resident pft_solve_ex.

    delta_mode: DELTA_GLOBAL (the driver's, intertrack.c:2165) or DELTA_LOCAL (the error norm times
    |h/3| before it is compared with delta, hybrid2.c:578).  chunk_mult: the chunk table's
    chunk_eps_mult (hybrid2.c:521) -- None (1, as the driver leaves them), three per-variable
    values (u, p, gl), or one value per chunk in the table's order (q, k, j; 3*n3*n2 of this
    slab).  It is written into self.chunk_mult after PrecalculateData, whose argument is that
    array (the reference's leaves it alone, equation.c:533, and so does libpft's: checked here),
    and before RK_MPI_SA_check_mem, so the solver sees it from its first call.
    """

    def __init__(self, n1, n2, total_n3, L, calc_mode, params, nprocs=1, rank=0, beads=None,
                 initial=None, tau=1.0, tau_min=0.0, delta=1e-3, t0=0.0, gl_static=False, kz=None,
                 init_solver=True, tile=None, recompute=True, icond=None, device_ic=False,
                 delta_mode=DELTA_GLOBAL, chunk_mult=None, icond_file=None):
        if delta_mode not in (DELTA_LOCAL, DELTA_GLOBAL):
            raise ValueError(f"delta_mode must be DELTA_LOCAL or DELTA_GLOBAL, not {delta_mode!r}")
        if icond_file is not None and (initial is not None or icond is not None or device_ic or not init_solver):
            # checked before any work: the file's state is read on the device of an initialised solver
            raise ValueError("icond_file reads the initial state from a snapshot dataset on the device: it cannot "
                             "be combined with initial=, icond=, device_ic or init_solver=False")
        if device_ic and (initial is not None or not init_solver):
            # checked before any host IC work: the device IC overwrites X/XN and the host copy
            raise ValueError("device_ic computes the IC (the default Params', or icond=) on an initialised "
                             "solver: it cannot be combined with initial= or init_solver=False")
        L1, L2, L3 = L
        self.lib = L_ = lib()
        if icond_file is not None:
            # the dataset's dimensions before any solver work: a region dataset, say (-4, the code
            # pft_solver_snapshot_read itself gives when it is asked)
            f1, f2, f3 = read_snapshot_info(icond_file)[:3]
            if (f1, f2, f3) != (n1, n2, total_n3):
                raise OSError(f"icond_file {icond_file}: the dataset's dimensions {f1}x{f2}x{f3} differ from the "
                              f"grid's {n1}x{n2}x{total_n3} (-4)")
        self.grid = pft_grid()
        rc = L_.pft_grid_init(C.byref(self.grid), n1, n2, total_n3, nprocs, rank, L1, L2, L3, calc_mode)
        if rc:
            raise ValueError(f"pft_grid_init failed ({rc})")
        self.params = np.ascontiguousarray(params, dtype=np.float64)
        if L_.pft_model_configure(C.byref(self.grid), _dp(self.params)):
            raise ValueError("pft_model_configure failed")
        g = self.grid
        self.N = (g.n3 + 4, g.n2 + 4, g.n1 + 4)
        self.S = int(np.prod(self.N))
        self.x = np.zeros(3 * self.S)
        # where the IC is computed: "device" (f1: the default IC, or icond programs that compile for
        # the device, pft_ic_compile), else "host"
        self.ic_where = "host"
        if device_ic and icond is not None:
            ok = []
            for q, prog in icond:
                ops = np.array([o for o, _ in prog], dtype=np.int32)
                args = np.array([a for _, a in prog], dtype=np.float64)
                ok.append(L_.pft_ic_device_ok(C.byref(self.grid), len(prog), _ip(ops), _dp(args)))
            if any(v < 0 for v in ok):
                raise ValueError(f"pft_ic_device_ok: a bad icond program ({ok})")
            device_ic = all(v == 1 for v in ok)   # one that is not device-exact: all on the host
        if device_ic or icond_file is not None:
            self.ic_where = "device"
        if icond_file is not None:
            pass                # read on the device after RK_MPI_SA_init (below)
        elif icond is not None and device_ic:
            pass                # the programs run on the device after RK_MPI_SA_init (below)
        elif icond is not None:
            # the parameter file's icond formulas, compiled by frontend.py (intertrack.c:1831-2012)
            for q, prog in icond:
                ops = np.array([o for o, _ in prog], dtype=np.int32)
                args = np.array([a for _, a in prog], dtype=np.float64)
                rc = L_.pft_ic_eval(C.byref(self.grid), q, len(prog), _ip(ops), _dp(args), _dp(self.x))
                if rc:
                    raise ValueError(f"pft_ic_eval failed ({rc})")
        elif initial is None:
            if not device_ic:   # (device_ic: computed on the device below, then downloaded)
                L_.pft_model_ic_default(_dp(self.x))
        else:
            self.set_interior(initial)
        nch = 3 * g.n2 * g.n3
        self.chunk_start = np.zeros(nch, dtype=np.int32)
        self.chunk_size = np.zeros(nch, dtype=np.int32)
        self.chunk_mult = np.zeros(nch, dtype=np.float64)
        L_.pft_model_chunks(_ip(self.chunk_start), _ip(self.chunk_size), _dp(self.chunk_mult))
        self.mem = RK_MEM_DIST(nch, _ip(self.chunk_start), _ip(self.chunk_size), _dp(self.chunk_mult))
        meta = {1: "mf_single"}.get(nprocs) or ("mf_bottom" if rank == 0 else
                                                ("mf_top" if rank == nprocs - 1 else "mf_middle"))
        self.meta_addr = C.cast(getattr(L_, meta), C.c_void_p).value
        self.system = RK_MPI_S_SOLUTION(C.pointer(self.mem), t0, _dp(self.x), self.meta_addr, tau,
                                        tau_min, delta, delta_mode, None, None, 0, 0)
        L_.pft_solver_set_option(PFT_OPT_GL_STATIC, 1 if gl_static else 0)
        L_.pft_solver_set_option(PFT_OPT_KZ, kz or 0)   # 0: automatic
        L_.pft_solver_set_option(PFT_OPT_TILE, 1 if tile is None else tile)   # 1: per stage
        L_.pft_solver_set_option(PFT_OPT_RECOMPUTE, 1 if recompute else 0)
        self.initialised = False
        if L_.AllocPrecalcData():
            raise RuntimeError("AllocPrecalcData failed")
        if beads is not None and initial is None:   # (also after icond formulas)
            b = np.ascontiguousarray(beads, dtype=np.float64)
            L_.pft_model_set_beads(_dp(b), b.shape[0])
            # device_ic: the beads are overlaid on the device (pft_solver_ic_default_device); on a
            # state from a file likewise (pft_solver_ic_beads_device)
            L_.pft_model_set_solution(None if device_ic or icond_file is not None else _dp(self.x))
        else:
            L_.pft_model_set_solution(None)
        if L_.PrecalculateData(_dp(self.chunk_mult)):
            raise RuntimeError("PrecalculateData failed")
        if not np.all(self.chunk_mult == 1.0):
            raise RuntimeError("PrecalculateData changed chunk_eps_mult")
        if chunk_mult is not None:
            cm = np.asarray(chunk_mult, dtype=np.float64)
            if cm.size == 3:
                cm = np.repeat(cm.reshape(3), g.n3 * g.n2)
            if cm.size != nch:
                raise ValueError(f"chunk_mult: 3 or {nch} values (q, k, j), not {cm.size}")
            self.chunk_mult[:] = cm.reshape(-1)     # in place: self.mem points at this array
        if init_solver:
            rc = L_.RK_MPI_SA_init(3 * self.S, MPI_COMM_WORLD, 0)
            if rc:
                raise RuntimeError(f"RK_MPI_SA_init failed ({rc})")
            self.initialised = True
            rc = L_.RK_MPI_SA_check_mem(C.byref(self.mem))
            if rc:
                raise RuntimeError(f"RK_MPI_SA_check_mem failed ({rc})")
        if device_ic:
            # f1: the default Params' IC (or the icond programs) and the beads computed on the device
            # (bit for bit the host's); the host array receives a copy, so every later call works
            # as after a host IC
            if icond is not None:
                qs = np.array([q for q, _ in icond], dtype=np.int32)
                lens = np.array([len(prog) for _, prog in icond], dtype=np.int32)
                ops = np.array([o for _, prog in icond for o, _ in prog], dtype=np.int32)
                args = np.array([a for _, prog in icond for _, a in prog], dtype=np.float64)
                rc = L_.pft_solver_ic_formulas_device(len(icond), _ip(qs), _ip(lens), _ip(ops), _dp(args),
                                                      1 if beads is not None else 0)
            else:
                rc = L_.pft_solver_ic_default_device(1 if beads is not None else 0)
            if rc:
                raise RuntimeError(f"pft_solver_ic_default_device failed ({rc}): {L_.pft_hip_last_error()}")
            if L_.pft_solver_download(C.byref(self.system)):
                raise RuntimeError("pft_solver_download failed")
        self._snap_pending = False
        if icond_file is not None:
            # f7: the state of a snapshot dataset read on the device, every rank its own planes
            # (icond_file, intertrack.c:2023-2117); the reference overlays the beads on it too
            # (equation.c:507-530); the host array receives a copy, as with device_ic
            rc = L_.pft_solver_snapshot_read(os.fsencode(icond_file))
            if rc:
                self.close()
                raise OSError(f"pft_solver_snapshot_read({icond_file}) failed ({rc}): {L_.pft_hip_last_error()}")
            if beads is not None:
                rc = L_.pft_solver_ic_beads_device()
                if rc:
                    self.close()
                    raise RuntimeError(f"pft_solver_ic_beads_device failed ({rc}): {L_.pft_hip_last_error()}")
            if L_.pft_solver_download(C.byref(self.system)):
                raise RuntimeError("pft_solver_download failed")

    # -- host array views ------------------------------------------------------------------
    def padded(self):
        return self.x.reshape((3,) + self.N)

    def interior(self):
        g = self.grid
        return np.ascontiguousarray(self.padded()[:, 2:2 + g.n3, 2:2 + g.n2, 2:2 + g.n1])

    def set_interior(self, a):
        """a: this slab's interior [3][n3][n2][n1], or the global [3][total_n3][n2][n1]"""
        g = self.grid
        if a.shape[1] != g.n3:
            a = a[:, g.first_row:g.first_row + g.n3]
        self.padded()[:, 2:2 + g.n3, 2:2 + g.n2, 2:2 + g.n1] = a

    # -- solving ---------------------------------------------------------------------------
    def solve(self, final_time):
        rc = self.lib.RK_MPI_SA_solve(final_time, C.byref(self.system))
        if rc < 0:
            raise RuntimeError(f"RK_MPI_SA_solve failed ({rc}): {self.lib.pft_hip_last_error()}")
        return rc

    def solve_ex(self, final_time, max_steps_total=0, flags=0):
        rc = self.lib.pft_solve_ex(final_time, C.byref(self.system), max_steps_total, flags)
        if rc < 0:
            raise RuntimeError(f"pft_solve_ex failed ({rc}): {self.lib.pft_hip_last_error()}")
        return rc

    def download(self):
        rc = self.lib.pft_solver_download(C.byref(self.system))
        if rc:
            raise RuntimeError(f"pft_solver_download failed ({rc})")

    # -- what the four reductions (f5, f6, f12, f13) share ---------------------------------------
    def _gather_bytes(self, raw):
        """every rank's `raw` (the same length on all of them) as a list of bytes in rank order
        (collective: pft_comm_allgather_any makes the rounds); a single rank makes no collective"""
        L_ = self.lib
        comm = L_.pft_comm_current()
        n = L_.pft_comm_size(comm) if comm else 1
        if n == 1:
            return [raw]
        every = C.create_string_buffer(n * len(raw))
        rc = L_.pft_comm_allgather_any(comm, raw, len(raw), every)
        if rc:
            raise RuntimeError(f"pft_comm_allgather failed ({rc})")
        return [every.raw[r * len(raw):(r + 1) * len(raw)] for r in range(n)]

    @staticmethod
    def _answer(entry, where, make):
        """make()'s answer for the entry `entry` after the check of `where`; RuntimeError when it is None
        (where="device" and nothing resident: the solver's -3, the same on every rank)"""
        _check_where(where)
        d = make()
        if d is None:
            raise RuntimeError(f"{entry}: no state is resident on the device (no initialised solver, or no "
                               "fused solve or device IC yet); solve first, or use where='host'")
        return d

    # -- f5: diagnostics and the driver's snapshot loop ------------------------------------------
    def _diag_host_global(self, o, planes):
        """pft_diag_host of self.x, merged over the communicator's ranks in rank order (collective)"""
        L_ = self.lib
        mine = pft_diag()
        rc = L_.pft_diag_host(C.byref(self.grid), _dp(self.x), C.byref(o), C.byref(mine), planes)
        if rc:
            raise RuntimeError(f"pft_diag_host failed ({rc})")
        parts = self._gather_bytes(bytes(mine))
        glob = pft_diag.from_buffer_copy(parts[0])
        for part in parts[1:]:
            L_.pft_diag_combine(C.byref(glob), C.byref(pft_diag.from_buffer_copy(part)))
        return glob, mine

    def diagnostics(self, p_thr=0.5, gl_thr=0.5, where="device", per_plane=False):
        """The ice diagnostics (include/pft_diag.h) of the whole grid as a dict: the struct's fields
        and ice_fraction = ice / cells, the published quantity (scripts/avg.sh).  where="device":
        of the device-resident state, by pft_solver_diag -- no download; collective on several
        ranks; RuntimeError when nothing is resident (before the first fused solve with a host
        IC).  where="host": pft_diag_host of self.x, merged over the ranks (collective too).
        per_plane: also ice_per_plane (this rank's planes) and first_row, and "local", this
        slab's own record."""
        return self._answer("diagnostics", where, lambda: self._diagnostics(p_thr, gl_thr, where, per_plane))

    def _diagnostics(self, p_thr, gl_thr, where, per_plane):
        """diagnostics(); None when where="device" and nothing is resident (pft_solver_diag's -3,
        the same on every rank)"""
        o = pft_diag_opts(p_thr, gl_thr)
        planes = (C.c_longlong * self.grid.n3)() if per_plane else None
        if where == "host":
            glob, mine = self._diag_host_global(o, planes)
        else:
            glob, mine = pft_diag(), pft_diag()
            rc = self.lib.pft_solver_diag(C.byref(o), C.byref(glob), C.byref(mine), planes)
            if rc == -3:
                return None
            if rc:
                raise RuntimeError(f"pft_solver_diag failed ({rc}): {self.lib.pft_hip_last_error()}")
        d = glob.as_dict()
        if per_plane:
            d["ice_per_plane"] = np.array(planes[:], dtype=np.int64)
            d["first_row"] = self.grid.first_row
            d["local"] = mine.as_dict()
        return d

    # -- f6: exact means and z-profiles ----------------------------------------------------------
    def _means_host_global(self, o, planes):
        """pft_means_host of self.x, merged over the communicator's ranks in rank order (collective)"""
        L_ = self.lib
        mine = pft_means()
        rc = L_.pft_means_host(C.byref(self.grid), _dp(self.x), C.byref(o), C.byref(mine), planes)
        if rc:
            raise RuntimeError(f"pft_means_host failed ({rc})")
        parts = self._gather_bytes(bytes(mine))
        glob = pft_means.from_buffer_copy(parts[0])
        for part in parts[1:]:
            L_.pft_means_combine(C.byref(glob), C.byref(pft_means.from_buffer_copy(part)))
        return glob, mine

    def means(self, p_thr=0.5, gl_thr=0.5, where="device", per_plane=False):
        """The exact means (include/pft_means.h) of the whole grid as a dict: for u (all cells), p
        (all cells), ice_u (u where p > p_thr) and pore_p (p where gl < gl_thr) the count *_n of
        the cells that entered, *_sum, the exact sum rounded once, and *_mean, the exact quotient
        rounded once (NaN when *_n is 0) -- the same bits on any decomposition.  where="device":
        of the device-resident state, by pft_solver_means -- no download; collective on several
        ranks; RuntimeError when nothing is resident.  where="host": pft_means_host of self.x,
        merged over the ranks (collective too).  per_plane: also u_profile, p_profile,
        ice_u_profile and pore_p_profile, the means of each of this rank's planes (global rows
        first_row + k), first_row, "local", this slab's own scalars, and "record" /
        "plane_records", the raw pft_means structs."""
        return self._answer("means", where, lambda: self._means(p_thr, gl_thr, where, per_plane))

    def _means(self, p_thr, gl_thr, where, per_plane):
        """means(); None when where="device" and nothing is resident (pft_solver_means' -3, the
        same on every rank)"""
        o = pft_diag_opts(p_thr, gl_thr)
        planes = (pft_means * self.grid.n3)() if per_plane else None
        if where == "host":
            glob, mine = self._means_host_global(o, planes)
        else:
            glob, mine = pft_means(), pft_means()
            rc = self.lib.pft_solver_means(C.byref(o), C.byref(glob), C.byref(mine), planes)
            if rc == -3:
                return None
            if rc:
                raise RuntimeError(f"pft_solver_means failed ({rc}): {self.lib.pft_hip_last_error()}")
        d = glob.as_dict()
        if per_plane:
            for q, k in enumerate(MEAN_KEYS):
                d[k + "_profile"] = np.array([m.values(q)[2] for m in planes], dtype=np.float64)
            d["first_row"] = self.grid.first_row
            d["local"] = mine.as_dict()
            d["record"] = glob
            d["plane_records"] = planes
        return d

    # -- f12: formula diagnostics ------------------------------------------------------------------
    def _formulas_host_global(self, progs, planes):
        """pft_formula_host of self.x, merged over the communicator's ranks in rank order (collective)"""
        L_ = self.lib
        names, lens, ops, args = progs
        nprog = len(names)
        mine = (pft_fdiag * nprog)()
        rc = L_.pft_formula_host(C.byref(self.grid), _dp(self.x), nprog, _ip(lens), _ip(ops), _dp(args), mine, planes)
        if rc:
            raise RuntimeError(f"pft_formula_host failed ({rc})")
        parts = self._gather_bytes(bytes(mine))
        glob = (pft_fdiag * nprog).from_buffer_copy(parts[0])
        for part in parts[1:]:
            other = (pft_fdiag * nprog).from_buffer_copy(part)
            for f in range(nprog):
                L_.pft_fdiag_combine(C.byref(glob[f]), C.byref(other[f]))
        return glob, mine

    def formulas(self, formulas, variables=None, where="device", per_plane=False):
        """f12: named formulas of the parameter file's language over the node inputs x, y, z, _x, _y,
        _z, u, p, gl and `variables` (a {name: value} dict or a frontend.Evaluator; the nine inputs
        always mean the node's own values), evaluated at every interior cell of the whole grid and
        reduced exactly (include/pft_formula.h).  Returns {name: dict} with cells, n, nonzero,
        nonfinite, min, max, maxabs, sum and mean -- the same bits on any decomposition.
        where="device": of the device-resident state, by pft_solver_formulas -- no download;
        collective on several ranks; RuntimeError when nothing is resident; ValueError naming the
        formula when one is not device-exact (pow or a libm function, C or P over a field or several
        coordinates, a deep stack: use where="host").  where="host": pft_formula_host of self.x,
        merged over the ranks (collective too); it accepts every formula.  per_plane: each dict
        also has <name>_profile, the means of this rank's planes (global rows first_row + k),
        first_row, "local", this slab's own scalars, and "record" / "plane_records", the raw
        pft_fdiag structs.  ValueError (frontend.EvalError is one) before any work for an undefined
        symbol, an empty dict, more than 8 formulas or programs of more than 256 entries."""
        return self._answer("formulas", where,
                            lambda: self._formulas(formula_programs(formulas, variables), where, per_plane))

    def _formula_not_exact(self, progs):
        """the name of the first formula that does not compile for the device, or None"""
        names, lens, ops, args = progs
        off = 0
        for name, n in zip(names, lens):
            pr = pft_ic_prog()
            rc = self.lib.pft_formula_compile(C.byref(self.grid), int(n), _ip(ops[off:off + n].copy()),
                                              _dp(args[off:off + n].copy()), C.byref(pr))
            self.lib.pft_ic_prog_free(C.byref(pr))
            if rc:
                return name
            off += int(n)
        return None

    def _formulas(self, progs, where, per_plane):
        """formulas() on compiled programs (formula_programs); None when where="device" and nothing
        is resident (pft_solver_formulas' -3, the same on every rank)"""
        names, lens, ops, args = progs
        nprog, n3 = len(names), self.grid.n3
        planes = (pft_fdiag * (n3 * nprog))() if per_plane else None
        if where == "host":
            glob, mine = self._formulas_host_global(progs, planes)
        else:
            glob, mine = (pft_fdiag * nprog)(), (pft_fdiag * nprog)()
            rc = self.lib.pft_solver_formulas(nprog, _ip(lens), _ip(ops), _dp(args), glob, mine, planes)
            if rc == -3:
                return None
            if rc == 1:
                raise ValueError(f"formulas: {self._formula_not_exact(progs)!r} is not device-exact (pow or a libm "
                                 "function, C or P over a field or several coordinates, or a stack deeper than "
                                 "the device's); use where='host'")
            if rc == -2:
                raise ValueError("formulas: pft_solver_formulas refused the programs (-2)")
            if rc:
                raise RuntimeError(f"pft_solver_formulas failed ({rc}): {self.lib.pft_hip_last_error()}")
        out = {}
        for f, name in enumerate(names):
            d = glob[f].as_dict()
            if per_plane:
                mine_planes = [planes[f * n3 + k] for k in range(n3)]
                d[name + "_profile"] = np.array([m.as_dict()["mean"] for m in mine_planes], dtype=np.float64)
                d["first_row"] = self.grid.first_row
                d["local"] = mine[f].as_dict()
                d["record"] = glob[f]
                d["plane_records"] = mine_planes
            out[name] = d
        return out

    # -- f13: histograms of formula values -----------------------------------------------------------
    def _hist_host_global(self, spec, plane_heads, plane_counts):
        """pft_hist_host of self.x, merged over the communicator's ranks in rank order (collective)"""
        L_ = self.lib
        edges = spec["edges"]
        nbins = edges.size - 1
        _, _, vops, vargs = spec["value"]
        value = pft_hist_prog(len(vops), _ip(vops), _dp(vargs))
        mask = None
        if spec["masked"] is not None:
            _, _, mops, margs = spec["masked"]
            mask = C.byref(pft_hist_prog(len(mops), _ip(mops), _dp(margs)))
        head, counts = pft_hist_head(), (C.c_longlong * nbins)()
        rc = L_.pft_hist_host(C.byref(self.grid), _dp(self.x), C.byref(value), mask, nbins, _dp(edges), C.byref(head),
                              counts, plane_heads, plane_counts)
        if rc:
            raise RuntimeError(f"pft_hist_host failed ({rc})")
        parts = self._gather_bytes(bytes(head) + bytes(counts))
        hs = C.sizeof(pft_hist_head)
        ghead = pft_hist_head.from_buffer_copy(parts[0][:hs])
        gcounts = (C.c_longlong * nbins).from_buffer_copy(parts[0][hs:])
        for part in parts[1:]:
            oh = pft_hist_head.from_buffer_copy(part[:hs])
            oc = (C.c_longlong * nbins).from_buffer_copy(part[hs:])
            L_.pft_hist_combine(nbins, C.byref(ghead), gcounts, C.byref(oh), oc)
        return (ghead, gcounts), (head, counts)

    def histogram(self, formula, bins, range=None, mask=None, variables=None, where="device", per_plane=False):
        """f13: the histogram of a formula of the parameter file's language (see formulas()) over the
        interior cells of the whole grid that the formula `mask` selects (value != 0, so a NaN
        selects; a math error does not; None: every cell) -- numpy.histogram(values[selected],
        bins=edges) with the NaN left out, by integer counts (include/pft_hist.h).  bins / range: see
        hist_edges().  Returns a dict: edges, counts (int64 [nbins]), under, over, nan, selected and
        cells, with selected == nan + under + over + counts.sum() -- the same numbers on any
        decomposition.  where="device": of the device-resident state, by pft_solver_hist -- no
        download; collective on several ranks; RuntimeError when nothing is resident; ValueError
        naming the formula when the formula or the mask is not device-exact (use where="host").
        where="host": pft_hist_host of self.x, merged over the ranks (collective too); it accepts
        every formula.  per_plane: also counts_per_plane (int64 [n3_local, nbins]), under_per_plane,
        over_per_plane, nan_per_plane, selected_per_plane (this rank's planes, global rows first_row
        + k), first_row and "local", this slab's own dict.  ValueError before any work for bad
        edges, an undefined symbol or a syntax error."""
        return self._answer("histogram", where,
                            lambda: self._histogram(hist_spec(formula, bins, range, mask, variables), where, per_plane))

    def _hist_not_exact(self, spec):
        """the text of the formula or mask that does not compile for the device, or None"""
        for what, progs in (("formula", spec["value"]), ("mask", spec["masked"])):
            if progs is not None and self._formula_not_exact(progs) is not None:
                return spec[what]
        return None

    def _histogram(self, spec, where, per_plane):
        """histogram() on a compiled spec (hist_spec); None when where="device" and nothing is
        resident (pft_solver_hist's -3, the same on every rank)"""
        edges = spec["edges"]
        nbins, n3 = edges.size - 1, self.grid.n3
        plane_heads = (pft_hist_head * n3)() if per_plane else None
        plane_counts = (C.c_longlong * (n3 * nbins))() if per_plane else None
        if where == "host":
            (ghead, gcounts), (lhead, lcounts) = self._hist_host_global(spec, plane_heads, plane_counts)
        else:
            _, _, vops, vargs = spec["value"]
            nm, mops, margs = 0, None, None
            if spec["masked"] is not None:
                _, _, mo, ma = spec["masked"]
                nm, mops, margs = len(mo), _ip(mo), _dp(ma)
            ghead, lhead = pft_hist_head(), pft_hist_head()
            gcounts, lcounts = (C.c_longlong * nbins)(), (C.c_longlong * nbins)()
            rc = self.lib.pft_solver_hist(len(vops), _ip(vops), _dp(vargs), nm, mops, margs, nbins, _dp(edges),
                                          C.byref(ghead), gcounts, C.byref(lhead), lcounts, plane_heads, plane_counts)
            if rc == -3:
                return None
            if rc == 1:
                raise ValueError(f"histogram: {self._hist_not_exact(spec)!r} is not device-exact (pow or a libm "
                                 "function, C or P over a field or several coordinates, or a stack deeper than "
                                 "the device's); use where='host'")
            if rc == -2:
                raise ValueError("histogram: pft_solver_hist refused the programs or the edges (-2)")
            if rc:
                raise RuntimeError(f"pft_solver_hist failed ({rc}): {self.lib.pft_hip_last_error()}")

        def as_dict(head, counts):
            d = {"edges": edges.copy(), "counts": np.array(counts[:], dtype=np.int64)}
            d.update(head.as_dict())
            return d

        d = as_dict(ghead, gcounts)
        if per_plane:
            d["counts_per_plane"] = np.array(plane_counts[:], dtype=np.int64).reshape(n3, nbins)
            for k in HIST_ROW_KEYS:
                d[k + "_per_plane"] = np.array([getattr(h, k) for h in plane_heads], dtype=np.int64)
            d["first_row"] = self.grid.first_row
            d["local"] = as_dict(lhead, lcounts)
        return d

    # -- f15: 2-D maps of formula values --------------------------------------------------------------
    def _map_neutral(self, n):
        a = np.zeros(n, dtype=MAP_DTYPE)
        a["min"], a["max"], a["first"], a["last"] = np.inf, -np.inf, -1, -1
        return a

    def _map_host_local(self, spec):
        """pft_map_host of self.x: this slab's records, flat"""
        _, _, vops, vargs = spec["value"]
        value = pft_hist_prog(len(vops), _ip(vops), _dp(vargs))
        mask = None
        if spec["masked"] is not None:
            _, _, mops, margs = spec["masked"]
            mask = C.byref(pft_hist_prog(len(mops), _ip(mops), _dp(margs)))
        rows, cols = self._map_dims(spec["axis"])
        out = np.empty(rows * cols, dtype=MAP_DTYPE)
        rc = self.lib.pft_map_host(C.byref(self.grid), _dp(self.x), C.byref(value), mask, spec["axis"], _map_ptr(out))
        if rc:
            raise RuntimeError(f"pft_map_host failed ({rc})")
        return out

    def _map_dims(self, axis):
        rows, cols = C.c_int(), C.c_int()
        if self.lib.pft_map_dims(C.byref(self.grid), axis, C.byref(rows), C.byref(cols)):
            raise ValueError(f"project: pft_map_dims refused axis {axis!r} (-2)")
        return rows.value, cols.value

    def _map_host_global(self, spec, local):
        """the ranks' host maps put together in rank order (collective), as pft_solver_map does it"""
        g, axis = self.grid, spec["axis"]
        rows, cols = self._map_dims(axis)
        if axis == 0:
            parts = self._gather_bytes(local.tobytes())
            glob = np.frombuffer(parts[0], dtype=MAP_DTYPE).copy()
            for part in parts[1:]:
                other = np.frombuffer(part, dtype=MAP_DTYPE).copy()
                self.lib.pft_map_combine(glob.size, _map_ptr(glob), _map_ptr(other))
            return glob
        places = [np.frombuffer(b, dtype=np.int64) for b in
                  self._gather_bytes(np.array([g.first_row, g.n3], dtype=np.int64).tobytes())]
        tallest = max(int(pl[1]) for pl in places)
        mine = self._map_neutral(tallest * cols)
        mine[:local.size] = local
        glob = self._map_neutral(g.total_n3 * cols)
        for pl, part in zip(places, self._gather_bytes(mine.tobytes())):
            at, n = int(pl[0]) * cols, int(pl[1]) * cols
            glob[at:at + n] = np.frombuffer(part, dtype=MAP_DTYPE)[:n]
        return glob

    def project(self, formula, axis, mask=None, variables=None, where="device", combine=True):
        """f15: a formula of the parameter file's language (see formulas()) reduced along one axis of
        the grid into a 2-D map (include/pft_map.h).  axis numbers interior()'s [k, j, i] as numpy
        does: 0 reduces z (the map is [n2, n1]), 1 reduces y ([total_n3, n1]), 2 reduces x
        ([total_n3, n2]).  Only the cells that the formula `mask` selects enter (value != 0, so a NaN
        selects; a math error does not; None: every cell).  Returns a dict of 2-D arrays: selected,
        nonzero (value != 0; a NaN counts), nonfinite (int64), min, max (float64, over the selected
        values that are not NaN; +inf / -inf where there is none), first, last (int64: the global
        index along the reduced axis of the first / last selected cell whose value is != 0, -1 where
        there is none); and "axis" and "rows" = (first_row, n3), the z range of the grid that the map
        covers.  With "p>0.5" along z, last is the front's height map and nonzero the ice thickness
        in cells.  Integers and ordered extrema only: the same bits on any decomposition.
        where="device": of the device-resident state, by pft_solver_map -- no download; collective
        on several ranks; RuntimeError when nothing is resident; ValueError naming the formula when
        the formula or the mask is not device-exact (use where="host").  where="host": pft_map_host
        of self.x, put together over the ranks (collective too); it accepts every formula.
        combine=False on several ranks: this slab's share alone -- its own rows for axes 1 and 2, its
        partial map for axis 0 -- and no map crosses between the ranks.  ValueError before any work
        for a bad axis, an undefined symbol or a syntax error."""
        return self._answer("project", where,
                            lambda: self._project(map_spec(formula, axis, mask, variables), where, combine))

    def _project(self, spec, where, combine=True):
        """project() on a compiled spec (map_spec); None when where="device" and nothing is resident
        (pft_solver_map's -3, the same on every rank)"""
        g, axis = self.grid, spec["axis"]
        rows, cols = self._map_dims(axis)
        comm = self.lib.pft_comm_current()
        several = bool(comm) and self.lib.pft_comm_size(comm) > 1
        glob = None
        if where == "host":
            local = self._map_host_local(spec)
            if several and combine:
                glob = self._map_host_global(spec, local)
        else:
            _, _, vops, vargs = spec["value"]
            nm, mops, margs = 0, None, None
            if spec["masked"] is not None:
                _, _, mo, ma = spec["masked"]
                nm, mops, margs = len(mo), _ip(mo), _dp(ma)
            local = np.empty(rows * cols, dtype=MAP_DTYPE)
            if several and combine:
                glob = np.empty((rows if axis == 0 else g.total_n3) * cols, dtype=MAP_DTYPE)
            rc = self.lib.pft_solver_map(len(vops), _ip(vops), _dp(vargs), nm, mops, margs, axis,
                                         None if glob is None else _map_ptr(glob), _map_ptr(local))
            if rc == -3:
                return None
            if rc == 1:
                raise ValueError(f"project: {self._hist_not_exact(spec)!r} is not device-exact (pow or a libm "
                                 "function, C or P over a field or several coordinates, or a stack deeper than "
                                 "the device's); use where='host'")
            if rc == -2:
                raise ValueError("project: pft_solver_map refused the programs or the axis (-2)")
            if rc:
                raise RuntimeError(f"pft_solver_map failed ({rc}): {self.lib.pft_hip_last_error()}")
        whole = glob is not None or not several
        a = (local if glob is None else glob).reshape(-1, cols)
        d = {k: np.ascontiguousarray(a[k]) for k in MAP_KEYS}
        d["axis"] = axis
        d["rows"] = (0, g.total_n3) if whole else (g.first_row, g.n3)
        return d

    # -- f7: snapshots from the resident state -----------------------------------------------------
    def _region(self, sel):
        """the pft_region of a selection (region()) on this simulation's grid; a pft_region is checked"""
        if isinstance(sel, pft_region):
            if self.lib.pft_region_check(C.byref(self.grid), C.byref(sel)):
                raise ValueError("region: the pft_region does not lie inside the grid")
            return sel
        try:
            k, j, i = sel
        except (TypeError, ValueError):
            raise ValueError(f"region: three items (k, j, i), each a slice or an int, not {sel!r}") from None
        return region(k, j, i, self.grid)

    def region_share(self, sel):
        """(kfirst, kcount, klocal) of pft_region_local: this slab's share of the region's k axis"""
        r, a, b, c = self._region(sel), C.c_int(), C.c_int(), C.c_int()
        rc = self.lib.pft_region_local(C.byref(self.grid), C.byref(r), C.byref(a), C.byref(b), C.byref(c))
        if rc:
            raise ValueError(f"pft_region_local failed ({rc})")
        return a.value, b.value, c.value

    def region(self, sel, where="device"):
        """f11: this rank's share of a region of the state, float64 [3][c3'][c2][c1] -- what
        interior()[:, k, j, i] holds for the slab's planes, ints kept as axes of length 1 (sel: see
        region()).  where="device": gathered on the device from the resident state
        (pft_solver_region: the region image through pinned memory, no file, no download of the
        rest); RuntimeError when nothing is resident.  where="host": the same from self.x."""
        _check_where(where)
        r = self._region(sel)
        _, kcount, klocal = self.region_share(r)
        out = np.zeros((3, kcount, r.count[1], r.count[0]))
        if where == "host":
            g = self.grid
            ks = slice(2 + klocal, 2 + klocal + kcount * r.stride[2], r.stride[2])
            js = slice(2 + r.start[1], 2 + r.start[1] + r.count[1] * r.stride[1], r.stride[1])
            is_ = slice(2 + r.start[0], 2 + r.start[0] + r.count[0] * r.stride[0], r.stride[0])
            out[...] = self.padded()[:, ks, js, is_][:, :kcount, :r.count[1], :r.count[0]]
            return out
        rc = self.lib.pft_solver_region(C.byref(r), _dp(out))
        if rc == -3:
            raise RuntimeError("region: no state is resident on the device (no initialised solver, or no fused "
                               "solve or device IC yet)")
        if rc:
            raise OSError(f"pft_solver_region failed ({rc}): {self.lib.pft_hip_last_error()}")
        return out

    def snapshot_device(self, path, info, wait=True, version=0, link=None, region=None):
        """Write the device-resident state as the snapshot dataset `path` (info: snapshot_info())
        without a download: the slab's image is byte-swapped on the device into pinned host memory
        and written by the library's background thread (pft_solver_snapshot_write; collective on
        several ranks).  wait=False returns once the image has left the device -- the next solve may
        run while the file is written; snapshot_wait() (or close()) then ends the write and reports
        its errors.  version: 0 automatic, 1 CDF-1, 2 CDF-2.  link: None (the default host link),
        "direct" or "staged".  RuntimeError when nothing is resident (no file is created).
        region=sel (f11; see region()): the dataset of the selected cells alone -- the same variables,
        attributes and coordinate variables, only smaller, plus the region_start / region_count /
        region_stride attributes -- gathered on the device: only the selection crosses to the host."""
        if link not in (None, "direct", "staged"):
            raise ValueError(f"link must be None, 'direct' or 'staged', not {link!r}")
        if version not in (0, 1, 2):
            raise ValueError(f"version must be 0, 1 or 2, not {version!r}")
        flags = (0 if wait else PFT_SNAP_ASYNC) | (version << 8)
        flags |= {None: 0, "direct": PFT_SNAP_DIRECT, "staged": PFT_SNAP_STAGED}[link]
        if region is not None:
            region = self._region(region)
        if not self._snapshot_device(path, info, flags, region):
            raise RuntimeError("snapshot_device: no state is resident on the device (no initialised solver, or "
                               "no fused solve or device IC yet)")

    def _snapshot_device(self, path, info, flags, region=None):
        """snapshot_device(); False when nothing is resident (pft_solver_snapshot_write's -3, the same
        on every rank, and no file); region: a pft_region or None"""
        if region is None:
            what = "pft_solver_snapshot_write"
            rc = self.lib.pft_solver_snapshot_write(os.fsencode(path), _dp(self.params), C.byref(info), flags)
        else:
            what = "pft_solver_snapshot_region_write"
            rc = self.lib.pft_solver_snapshot_region_write(os.fsencode(path), _dp(self.params), C.byref(info),
                                                           C.byref(region), flags)
        if rc == -3:
            return False
        if rc:
            raise OSError(f"{what}({path}) failed ({rc}): {self.lib.pft_hip_last_error()}")
        if flags & PFT_SNAP_ASYNC:
            self._snap_pending = True
        return True

    def snapshot_wait(self):
        """wait for the background writes of snapshot_device(wait=False); OSError for the first one
        that failed (collective on several ranks)"""
        self._snap_pending = False
        rc = self.lib.pft_solver_snapshot_wait()
        if rc:
            raise OSError(f"pft_solver_snapshot_wait: a background snapshot write failed ({rc})")

    def run_series(self, final_time=None, saved_files=None, times=None, snapshot_path=None, comment="",
                   diag=True, opts=None, means=False, snapshot_where="host", snapshot_async=False,
                   first_snapshot=0, total_snapshots=None, skip_first=False, regions=None, region_every=1,
                   snapshot_full=True, formulas=None, variables=None, histograms=None, maps=None, map_every=1):
        """The driver's snapshot loop (intertrack.c:2265-2283).  Snapshot 0 is the state as it
        stands (no solve); snapshot s solves to series_times(t0, final_time, saved_files)[s], or
        to times[s - 1] when times= lists the solve targets.  The steps run device-resident
        (pft_solve_ex with KEEP_DEVICE | REUSE_DEVICE: nothing crosses PCIe between snapshots; the
        first call uploads unless the IC is already on the device).  Returns one dict per
        snapshot: snapshot, t, h, steps, steps_total, rc (None for snapshot 0) and, with diag,
        the global diagnostics (opts: a (p_thr, gl_thr) pair); with means=True also the scalar
        keys of means() (u_mean, p_mean, ice_u_mean, pore_p_mean, their _sum and _n), so that
        write_series_txt(rows, path, key="u_mean") writes a series of them.  snapshot_path: every snapshot is
        also downloaded and written to "<snapshot_path>.%03d.ncd" with the reference's snapshot /
        total_snapshots attributes.  Collective on several ranks.  A solve that returns 1 (a
        Service_Callback break) ends the series with that row.
        snapshot_where="device": the files come from snapshot_device() -- no download; with
        snapshot_async each write overlaps the next interval's steps and the series ends with
        snapshot_wait().  first_snapshot=k continues a series (continue_series,
        intertrack.c:1642-1669, 2265-2271): the state as it stands is snapshot k of saved_files,
        rows and file names are numbered from k and the targets are series_times(..., first=k);
        snapshot k is written again unless skip_first (:2315).  total_snapshots: the files'
        attribute when times= is given (default: first_snapshot + the number of rows).
        regions={"xz": sel, ...} (f11; sel: see region()): each named region is written as the region
        dataset "<snapshot_path>.<name>.%03d.ncd" at every snapshot whose number is a multiple of
        region_every, by the route of snapshot_where and snapshot_async; snapshot_full=False leaves
        the full datasets out altogether.  The rows do not depend on any of it.
        formulas={name: expression} (f12; variables: see formulas(); or formula_programs()' result, compiled
        already): every row also carries
        <name>_mean, _sum, _n, _nonzero, _min, _max and _maxabs of each formula over the whole grid, from
        the device-resident state, so that write_series_txt(rows, path, key="<name>_mean") writes its
        series.  The programs are compiled once, before the first solve; ValueError up front for a
        formula that is not device-exact and for a name whose keys would collide with a key of
        diagnostics() or means().
        histograms={name: {"formula": ..., "bins": ..., "range": ..., "mask": ...}} (f13; range and mask
        optional, see histogram(); or hist_spec()'s result, compiled already): every row also carries
        <name>, the counts (int64 [nbins]) over the whole grid from the device-resident state, and
        <name>_under, _over, _nan and _selected, so that write_hist_txt(rows, path, key="<name>")
        writes the series.  The specs are compiled once, before the first solve; ValueError up front
        for bad edges, a formula or mask that is not device-exact and for a name whose keys collide
        with another key of the rows.  All other row keys are unchanged.
        maps={name: {"formula": ..., "axis": ..., "mask": ...}} (f15; mask optional, see project(); or
        map_spec()'s result, compiled already): every row of a snapshot whose number is a multiple of
        map_every also carries <name>, project()'s dict of the whole grid from the device-resident
        state; with snapshot_path that dict is also written as "<snapshot_path>.<name>.%03d.npz" (by
        rank 0).  The specs are compiled once, before the first solve; ValueError up front for a bad
        axis, a formula or mask that is not device-exact and for a name that collides with another
        key of the rows.  Rows without maps= are unchanged."""
        map_specs = None
        if maps is not None:
            if not isinstance(maps, dict) or not maps:
                raise ValueError("run_series: maps= is a non-empty {name: spec} dict")
            map_every = int(map_every)
            if map_every < 1:
                raise ValueError(f"map_every must be at least 1, not {map_every}")
            map_specs = {}
            for name, sp in maps.items():
                if not isinstance(sp, dict) or not (sp.get("compiled") or {"formula", "axis"} <= set(sp)):
                    raise ValueError(f"run_series: map {name!r} needs 'formula' and 'axis'")
                if not sp.get("compiled"):
                    extra = set(sp) - {"formula", "axis", "mask"}
                    if extra:
                        raise ValueError(f"run_series: map {name!r} has unknown keys {sorted(extra)}")
                    sp = map_spec(sp["formula"], sp["axis"], sp.get("mask"), variables)
                bad = self._hist_not_exact(sp)
                if bad is not None:
                    raise ValueError(f"run_series: map {name!r}: {bad!r} is not device-exact; evaluate it "
                                     "with project(where='host') on a downloaded state")
                map_specs[str(name)] = sp
        hists = None
        if histograms is not None:
            if not isinstance(histograms, dict) or not histograms:
                raise ValueError("run_series: histograms= is a non-empty {name: spec} dict")
            hists = {}
            for name, sp in histograms.items():
                if not isinstance(sp, dict) or not (sp.get("compiled") or {"formula", "bins"} <= set(sp)):
                    raise ValueError(f"run_series: histogram {name!r} needs 'formula' and 'bins'")
                if not sp.get("compiled"):
                    extra = set(sp) - {"formula", "bins", "range", "mask"}
                    if extra:
                        raise ValueError(f"run_series: histogram {name!r} has unknown keys {sorted(extra)}")
                    sp = hist_spec(sp["formula"], sp["bins"], sp.get("range"), sp.get("mask"), variables)
                bad = self._hist_not_exact(sp)
                if bad is not None:
                    raise ValueError(f"run_series: histogram {name!r}: {bad!r} is not device-exact; evaluate it "
                                     "with histogram(where='host') on a downloaded state")
                hists[str(name)] = sp
        progs = None
        if formulas is not None:
            # (a tuple: programs compiled already by formula_programs, as Case.run passes them)
            progs = formulas if isinstance(formulas, tuple) else formula_programs(formulas, variables)
            taken = self._series_keys()
            keys = [name + "_" + k for name in progs[0] for k in FORMULA_ROW_KEYS]
            clash = sorted(set(keys) & taken) + sorted({k for k in keys if keys.count(k) > 1})
            if clash:
                raise ValueError(f"run_series: the formula keys {clash} collide with keys of diagnostics(), "
                                 "means() or another formula; rename the formula")
            bad = self._formula_not_exact(progs)
            if bad is not None:
                raise ValueError(f"run_series: formula {bad!r} is not device-exact; evaluate it with "
                                 "formulas(where='host') on a downloaded state")
        if hists is not None:
            taken = self._series_keys()
            if progs is not None:
                taken |= {name + "_" + k for name in progs[0] for k in FORMULA_ROW_KEYS}
            keys = [k for name in hists for k in [name] + [name + "_" + s for s in HIST_ROW_KEYS]]
            clash = sorted(set(keys) & taken) + sorted({k for k in keys if keys.count(k) > 1})
            if clash:
                raise ValueError(f"run_series: the histogram keys {clash} collide with other keys of the rows; "
                                 "rename the histogram")
        if map_specs is not None:
            taken = self._series_keys()
            if progs is not None:
                taken |= {name + "_" + k for name in progs[0] for k in FORMULA_ROW_KEYS}
            if hists is not None:
                taken |= {k for name in hists for k in [name] + [name + "_" + s for s in HIST_ROW_KEYS]}
            clash = sorted(set(map_specs) & taken)
            if clash:
                raise ValueError(f"run_series: the map keys {clash} collide with other keys of the rows; "
                                 "rename the map")
        region_every = int(region_every)
        if region_every < 1:
            raise ValueError(f"region_every must be at least 1, not {region_every}")
        if regions and snapshot_path is None:
            raise ValueError("regions= needs snapshot_path")
        regions = {str(name): self._region(sel) for name, sel in (regions or {}).items()}
        if snapshot_where not in ("host", "device"):
            raise ValueError(f"snapshot_where must be 'host' or 'device', not {snapshot_where!r}")
        if snapshot_async and snapshot_where != "device":
            raise ValueError("snapshot_async needs snapshot_where='device'")
        first = int(first_snapshot)
        if first < 0:
            raise ValueError(f"first_snapshot must not be negative, not {first_snapshot}")
        t0 = self.system.t
        if times is not None:
            targets = [t0] + [float(t) for t in times]
        else:
            if final_time is None or saved_files is None:
                raise ValueError("run_series needs final_time and saved_files, or times=")
            targets = series_times(t0, final_time, saved_files, first)
        total = first + len(targets) if total_snapshots is None else int(total_snapshots)
        p_thr, gl_thr = opts if opts is not None else (0.5, 0.5)
        end = targets[-1] if final_time is None else float(final_time)
        rows = []
        try:
            rows = self._run_series(targets, first, total, end, p_thr, gl_thr, snapshot_path, comment, diag, means,
                                    snapshot_where, snapshot_async, skip_first, regions, region_every, snapshot_full,
                                    progs, hists, map_specs, map_every)
        finally:
            if self._snap_pending:
                self.snapshot_wait()
        return rows

    @staticmethod
    def _series_keys():
        """the row keys of run_series without formulas= and histograms="""
        return ({"snapshot", "t", "h", "steps", "steps_total", "rc", "ice_fraction"}
                | {k for k, _ in pft_diag._fields_} | {k + s for k in MEAN_KEYS for s in ("_n", "_sum", "_mean")})

    def _run_series(self, targets, first, total, end, p_thr, gl_thr, snapshot_path, comment, diag, means,
                    snapshot_where, snapshot_async, skip_first, regions, region_every, snapshot_full, progs=None,
                    hists=None, map_specs=None, map_every=1):
        not_resident = ("run_series: no state is resident on the device after the solve "
                        "(the host-staged path keeps none)")

        def resident(call, *args):
            """the device's answer; at the first snapshot of a host IC, whose state is still the host
            array, the host's"""
            d = call(*args, "device", False)
            if d is None and s == first:
                d = call(*args, "host", False)
            if d is None:
                raise RuntimeError(not_resident)
            return d

        rows = []
        for s, T in enumerate(targets, first):
            rc = None
            if s > first:
                rc = self.solve_ex(T, 0, PFT_SOLVE_KEEP_DEVICE | PFT_SOLVE_REUSE_DEVICE)
            row = {"snapshot": s, "t": self.system.t, "h": self.system.h, "steps": self.system.steps,
                   "steps_total": self.system.steps_total, "rc": rc}
            if diag:
                row.update(resident(self._diagnostics, p_thr, gl_thr))
            if means:
                row.update(resident(self._means, p_thr, gl_thr))
            if progs is not None:
                for name, rec in resident(self._formulas, progs).items():
                    row.update({name + "_" + k: rec[k] for k in FORMULA_ROW_KEYS})
            for name, sp in (hists or {}).items():
                d = resident(self._histogram, sp)
                row[name] = d["counts"]
                row.update({name + "_" + k: d[k] for k in HIST_ROW_KEYS})
            if s % map_every == 0:
                for name, sp in (map_specs or {}).items():
                    d = resident(lambda spec, where, _planes: self._project(spec, where, True), sp)
                    row[name] = d
                    if snapshot_path is not None and self.grid.rank == 0:
                        np.savez("%s.%s.%03d.npz" % (snapshot_path, name, s), **d)
            if snapshot_path is not None and not (s == first and skip_first):
                info = snapshot_info(self.system.t, self.system.h, end, self.system.delta, self.grid.calc_mode,
                                     snapshot=s, total_snapshots=total, comment=comment)
                files = [("%s.%03d.ncd" % (snapshot_path, s), None)] if snapshot_full else []
                if s % region_every == 0:
                    files += [("%s.%s.%03d.ncd" % (snapshot_path, name, s), reg) for name, reg in regions.items()]
                downloaded = False
                for name, reg in files:
                    written = False
                    if snapshot_where == "device":
                        written = self._snapshot_device(name, info, PFT_SNAP_ASYNC if snapshot_async else 0, reg)
                        if not written and s != first:
                            raise RuntimeError(not_resident)
                    if not written:
                        # the host path; with "device" the first snapshot of a host IC, not yet resident
                        if not downloaded:
                            drc = self.lib.pft_solver_download(C.byref(self.system))
                            if drc and not (drc == -2 and s == first):   # -2 at the first: a host IC, nothing resident yet
                                raise RuntimeError(f"pft_solver_download failed ({drc})")
                            downloaded = True
                        save_snapshot(self, name, info, region=reg)
            rows.append(row)
            if rc == 1:
                break
        return rows

    def tile_geometry(self):
        """{stage: (kernel kind, wx cell pairs, ty rows)} of the slab's stage launches (kind 0 cache,
        1 LDS tile with aux arrays, 2 fused recompute); the slab exists after the first solve"""
        slab = self.lib.pft_solver_slab()
        if not slab:
            return None
        out = {}
        for st in range(1, 6):
            wx, ty = C.c_int(), C.c_int()
            kind = self.lib.pft_slab_tile_geometry(slab, st, C.byref(wx), C.byref(ty))
            out[st] = (kind, wx.value, ty.value)
        return out

    def stats(self):
        s = pft_solver_stats()
        self.lib.pft_solver_get_stats(C.byref(s))
        return s

    @property
    def t(self):
        return self.system.t

    @property
    def h(self):
        return self.system.h

    def close(self):
        if getattr(self, "_snap_pending", False):
            # the background writer still reads the slab's pinned image
            self._snap_pending = False
            self.lib.pft_solver_snapshot_wait()
        if self.initialised:
            self.lib.RK_MPI_SA_cleanup()
            self.initialised = False
        self.lib.FreePrecalcData()


def snapshot_info(t, tau, final_time, delta, calc_mode, snapshot=0, total_snapshots=0, comment=""):
    """pft_snapshot_info; its title is the reference's "Intertrack simulation (<comment>). Time: <t>"."""
    info = pft_snapshot_info(t, tau, final_time, delta, snapshot, total_snapshots, calc_mode)
    info.title = ("Intertrack simulation (%s). Time: %g" % (comment, t)).encode()[:255]   # C's %g
    return info


def save_snapshot(sim, path, info, region=None, version=0):
    """Write this slab's part of a NetCDF-classic snapshot (pft_io.h); the host array must hold the
    state (Simulation.download() after a device-resident solve).  Multi-rank: every rank calls it.
    region=sel (f11; see region()): the region dataset of the selected cells instead, byte for byte
    what Simulation.snapshot_device(region=sel) writes from the resident state; version (1: CDF-1,
    2: CDF-2, 0: automatic) is taken with a region only."""
    if region is None:
        if version:
            raise ValueError("save_snapshot: version= is taken with region= only")
        rc = lib().pft_snapshot_write(os.fsencode(path), C.byref(sim.grid), _dp(sim.params), C.byref(info), _dp(sim.x))
        if rc:
            raise OSError(f"pft_snapshot_write({path}) failed ({rc})")
        return
    if version not in (0, 1, 2):
        raise ValueError(f"version must be 0, 1 or 2, not {version!r}")
    r = sim._region(region)
    rc = lib().pft_snapshot_write_region(os.fsencode(path), C.byref(sim.grid), C.byref(r), _dp(sim.params),
                                         C.byref(info), _dp(sim.x), version)
    if rc:
        raise OSError(f"pft_snapshot_write_region({path}) failed ({rc})")


def read_snapshot_info(path):
    """(n1, n2, total_n3, pft_snapshot_info, params[PFT_PARAM_COUNT]) of a snapshot dataset"""
    n1, n2, n3 = C.c_int(), C.c_int(), C.c_int()
    info = pft_snapshot_info()
    prm = np.full(len(PARAM_NAMES), np.nan)
    rc = lib().pft_snapshot_read_info(os.fsencode(path), C.byref(n1), C.byref(n2), C.byref(n3), C.byref(info), _dp(prm))
    if rc:
        raise OSError(f"pft_snapshot_read_info({path}) failed ({rc})")
    return n1.value, n2.value, n3.value, info, prm


def read_snapshot_series(path):
    """(rc, snapshot, total_snapshots, t, final_time, tau): the attributes a continued series starts
    from (pft_snapshot_read_series); rc -3 when one of them is missing, other codes as pft_io.h"""
    snap, total = C.c_int(), C.c_int()
    t, final, tau = C.c_double(), C.c_double(), C.c_double()
    rc = lib().pft_snapshot_read_series(os.fsencode(path), C.byref(snap), C.byref(total), C.byref(t),
                                        C.byref(final), C.byref(tau))
    return rc, snap.value, total.value, t.value, final.value, tau.value


def load_snapshot(sim, path):
    """Fill this slab's interior from a snapshot dataset (restart / icond_file, intertrack.c:2040-2069)"""
    rc = lib().pft_snapshot_read_slab(os.fsencode(path), C.byref(sim.grid), _dp(sim.x))
    if rc:
        raise OSError(f"pft_snapshot_read_slab({path}) failed ({rc})")


def rhs(sim, t, state_padded=None):
    """K = f(t, w) through the model's RHS meta-pointer (equation.c contract) on host arrays."""
    L_ = sim.lib
    w = sim.x.copy() if state_padded is None else np.ascontiguousarray(state_padded, dtype=np.float64)
    dw = np.zeros_like(w)
    fname = "f_generic_model2" if sim.grid.calc_mode == 2 else "f_generic_model01"
    getattr(L_, fname)(t, _dp(w), _dp(dw))
    return dw, w


def _cosh_call(name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    fn = getattr(lib(), name)
    fn.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_ulonglong]
    rc = fn(_dp(x.reshape(-1)), _dp(y.reshape(-1)), x.size)
    if rc:
        raise RuntimeError(f"{name} failed ({rc}): {lib().pft_hip_last_error().decode()}")
    return y


def cosh_device(x):
    """calc_mode 2's cosh (csrc/pft_cosh.h) of every element of x, evaluated on the GPU"""
    return _cosh_call("pft_cosh_eval", x)


def cosh_host(x):
    """the same code compiled for the host: bit for bit cosh_device and x86-64 glibc's cosh"""
    return _cosh_call("pft_cosh_host", x)
