"""Helpers of tests/test_schur_variants_gpu.py and tests/test_schur_variant_systems_host.py: BA systems with designed
visibility -- every landmark's camera list is written down, so that the host analysis of the landmark-major assembly
(schur_tile_routes, csrc/schur_tile_tables.cpp) meets the job shape a case is about --, their dense high-precision references
(never the library under test), the analysis' rules restated (which jobs a run of landmarks becomes), the parser of the
"[schur report]" lines the analysis prints under SLAMPP_HIP_PLAN_TIMING, and the one list of checks every case goes through.

Nothing GPU-bound is imported at module level: the systems and references are built at first use and kept.
DESIGN.md ("Which test guards which branch of the Schur assembly") maps instantiation -> gate -> test id."""
import collections
import dataclasses
import re

import numpy as np

from slam_plus_plus_amd import synth

TOL = 1e-10                            # the project's bound on ||x - x_ref||_inf / ||x_ref||_inf
ORACLE_TOL = 1e-12                     # the CPU oracle against the refined reference: two orders below TOL
COND_MAX = 1e6                         # cond_2(Lambda) of every fixture
DAMPING = 0.1                          # synth.ba's default: the fixtures' cond_2 stays under COND_MAX with it (host test)
DIMS = [(6, 3), (7, 3), (3, 2)]        # (cam_dim, pt_dim) the Schur kernels are compiled for
TILE_SLOTS, TILE_POINTS, TILE_MAX_K = 64, 64, 10   # schur_tiles.h: SCHUR_TILE_SLOTS, SCHUR_TILE_MAX_POINTS; tile_max_k(64)
# first and last k of every bucket of NT = (min(k, OB) DC + 15) / 16 (16-line matrix-core tiles a side of a run job)
NT_BUCKETS = {6: [(1, 2), (3, 5), (6, 8), (9, 10)], 7: [(1, 2), (3, 4), (5, 6), (7, 9)], 3: [(1, 5), (6, 10), (11, 16), (17, 21)]}


def rel_inf(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def ob_of(dc):
    """Observations a block of a run job holds (OB in schur_tiles.hip)."""
    return 64 // dc


def nt_of(dc, k):
    """class_tiles of read_class_lists() (csrc/schur_tile_tables.cpp): 16-line tiles a side of a landmark's first job."""
    return (min(k, ob_of(dc)) * dc + 15) // 16


def tile_loads(dc, dp, k_max):
    """tile_launch_loads() of schur_tiles.hip: NL of the tile kernel for a largest landmark of k_max cameras."""
    nl_max = (TILE_MAX_K * dc * dp + 63) // 64
    return max(1, min((k_max * dc * dp + 63) // 64, 4, nl_max))


# ---- the builder ----------------------------------------------------------------------------------------------------------------

def build_system(cam_lists, cam_dim, pt_dim, seed=0, damping=DAMPING, n_cams=None, name="ba_designed"):
    """A BA system whose landmark p is seen by exactly the cameras ``cam_lists[p]`` (sorted, distinct; an empty list is a
    landmark nobody sees), in the layout synth.ba writes -- cameras first, per landmark its U blocks (by camera) and then C,
    blocks column-major -- and with its recipe for the values: per observation Jc in R^{2 x cam_dim}, Jp in R^{2 x pt_dim}
    ~ N(0, 1), A_cc += Jc^T Jc, C_pp += Jp^T Jp, U_cp = Jc^T Jp, ``damping`` I on every diagonal block, eta ~ N(0, 1)."""
    lists = [np.asarray(l, dtype=np.int64).reshape(-1) for l in cam_lists]
    for l in lists:
        assert l.size == 0 or (np.all(np.diff(l) > 0) and l[0] >= 0), "camera lists are sorted and distinct"
    n_pts = len(lists)
    kk = np.array([l.size for l in lists], dtype=np.int64)
    cam_s = np.concatenate(lists) if n_pts and kk.sum() else np.zeros(0, dtype=np.int64)
    if n_cams is None:
        n_cams = int(cam_s.max()) + 1
    assert cam_s.size and cam_s.max() < n_cams
    pt_s = np.repeat(np.arange(n_pts), kk)
    n_obs = int(kk.sum())
    rng = np.random.default_rng(seed)
    cd, pd_ = cam_dim, pt_dim
    Jc = rng.standard_normal((n_obs, 2, cd))
    Jp = rng.standard_normal((n_obs, 2, pd_))
    Acc = synth._segment_sum(cam_s, np.einsum("oki,okj->oij", Jc, Jc), n_cams)
    Cpp = synth._segment_sum(pt_s, np.einsum("oki,okj->oij", Jp, Jp), n_pts)
    U_s = np.einsum("oki,okj->oij", Jc, Jp)                 # [n_obs, cd, pd]: already in storage order
    Acc += damping * np.eye(cd)[None]
    Cpp += damping * np.eye(pd_)[None]
    n_bc = n_cams + n_pts
    bcol_ptr = np.zeros(n_bc + 1, dtype=np.int64)
    bcol_ptr[1:n_cams + 1] = np.arange(1, n_cams + 1)
    np.cumsum(kk + 1, out=bcol_ptr[n_cams + 1:])
    bcol_ptr[n_cams + 1:] += n_cams
    nb = int(bcol_ptr[-1])
    brow = np.empty(nb, dtype=np.int32)
    brow[:n_cams] = np.arange(n_cams)
    diag_pos = bcol_ptr[n_cams + 1:] - 1
    brow[diag_pos] = n_cams + np.arange(n_pts, dtype=np.int32)
    mask = np.ones(nb, dtype=bool)
    mask[:n_cams] = False
    mask[diag_pos] = False
    brow[np.nonzero(mask)[0]] = cam_s
    sz = np.empty(nb, dtype=np.int64)
    sz[:n_cams] = cd * cd
    sz[diag_pos] = pd_ * pd_
    sz[mask] = cd * pd_
    vals = np.empty(int(sz.sum()))
    n_a = n_cams * cd * cd
    vals[:n_a] = Acc.transpose(0, 2, 1).ravel()
    scalar_is_u = np.repeat(mask[n_cams:], sz[n_cams:])
    pts = vals[n_a:]
    pts[scalar_is_u] = U_s.transpose(0, 2, 1).ravel()
    pts[~scalar_is_u] = Cpp.transpose(0, 2, 1).ravel()
    cumsum = np.concatenate([np.arange(n_cams + 1, dtype=np.int64) * cd,
                             n_cams * cd + np.arange(1, n_pts + 1, dtype=np.int64) * pd_])
    rhs = rng.standard_normal(int(cumsum[-1]))
    return synth.BlockSystem(cumsum, bcol_ptr, brow, vals, rhs, n_cams, name)


def camera_lists(lam):
    """The camera list of every landmark of a BA system, as build_system() takes them."""
    nc = lam.n_matrix_cut
    return [lam.brow_idx[lam.bcol_ptr[nc + p]:lam.bcol_ptr[nc + p + 1] - 1].astype(np.int64) for p in range(lam.n_bcols - nc)]


def dense(lam):
    return lam.to_scipy().toarray()


def refined_solutions(A, B):
    """X of A X = B for the columns of B: dense LU in fp64, then two steps of iterative refinement with the residuals
    B - A X accumulated in long double (what variant_util.refined_solution does, on the dense Lambda)."""
    import scipy.linalg as sla
    lu = sla.lu_factor(A)
    ld = np.longdouble
    A_ld, B_ld = A.astype(ld), B.astype(ld)
    X = sla.lu_solve(lu, B)
    for _ in range(2):
        R = B_ld - A_ld @ X.astype(ld)
        X = X + sla.lu_solve(lu, R.astype(np.float64))
    return X


def with_changed_landmark(lam, p, rng):
    """The system after a relinearization that moved landmark ``p``: its U blocks and C change, and so do every camera's
    diagonal block (a little more on the diagonal) and the whole right-hand side."""
    nc = lam.n_matrix_cut
    off = lam.block_value_offsets()
    vals = lam.values.copy()
    k0, k1 = int(lam.bcol_ptr[nc + p]), int(lam.bcol_ptr[nc + p + 1])
    for k in range(k0, k1 - 1):
        vals[off[k]:off[k + 1]] *= 1.0 - 0.5 * rng.random()          # (smaller U, larger C and A: still positive definite)
    d = int(lam.cumsum[nc + p + 1] - lam.cumsum[nc + p])
    vals[off[k1 - 1]:off[k1]] += (0.5 + rng.random()) * np.eye(d).ravel()
    for c in range(nc):
        k = int(lam.bcol_ptr[c + 1] - 1)
        d = int(lam.cumsum[c + 1] - lam.cumsum[c])
        vals[off[k]:off[k + 1]] += (0.1 + rng.random()) * np.eye(d).ravel()
    return dataclasses.replace(lam, values=vals, rhs=rng.standard_normal(lam.rhs.shape[0]))


def with_indefinite_landmark(lam, p):
    """A copy with 4 max|C| I subtracted from C of landmark ``p``: every eigenvalue of the block is negative then."""
    nc = lam.n_matrix_cut
    off = lam.block_value_offsets()
    k1 = int(lam.bcol_ptr[nc + p + 1])
    d = int(lam.cumsum[nc + p + 1] - lam.cumsum[nc + p])
    vals = lam.values.copy()
    vals[off[k1 - 1]:off[k1]] -= 4.0 * np.abs(vals[off[k1 - 1]:off[k1]]).max() * np.eye(d).ravel()
    return dataclasses.replace(lam, values=vals)


# ---- the analysis' rules, restated ------------------------------------------------------------------------------------------

def run_jobs(dc, members_k, mult=1):
    """CRunEmitter::Emit_Run() (csrc/schur_tile_tables.cpp) for one run whose members have ``members_k`` cameras (longest first): a Counter over
    (NT, diagonal, prefix, landmarks of the job).  Pieces of 64 landmarks -- 32 where a job keeps more than three tiles a
    side --, ``mult`` times that with SLAMPP_HIP_DEV_RUN_PIECE_MULT; a job per pair (rb >= cb) of observation blocks, over
    the piece's landmarks that reach into row block rb."""
    ob = ob_of(dc)
    piece = (32 if min(members_k[0], ob) * dc > 48 else 64) * mult
    jobs = collections.Counter()
    for f in range(0, len(members_k), piece):
        ks = members_k[f:f + piece]
        k = ks[0]
        for rb in range((k + ob - 1) // ob):
            n_kb_r = min(ob, k - rb * ob)
            n_reach = sum(1 for q in ks if q > rb * ob)
            for cb in range(rb + 1):
                n_kb_c = min(ob, k - cb * ob)
                nt = (max(n_kb_r, n_kb_c) * dc + 15) // 16
                jobs[(nt, int(rb == cb), int(ks[n_reach - 1] < k), n_reach)] += 1
    return jobs


def launches_of(jobs, knobs):
    """The launches of tiles_enqueue_t for the jobs of every run together: {(NT, diagonal, prefix): {"quad", "jobs", "points":
    {landmarks of a job: jobs}}}.  Where a (NT, diagonal) class has one job whose landmarks end early, all its jobs run the
    masking instance; quads wherever a job stages a multiple of four landmarks (run_launch_quad)."""
    masked = {(nt, d) for (nt, d, x, _), c in jobs.items() if x}
    out = {}
    for (nt, d, x, n), c in jobs.items():
        key = (nt, d, int((nt, d) in masked))
        quad = (nt <= 2 or (d and "SLAMPP_HIP_DEV_NO_QUAD_WIDE" not in knobs)) and "SLAMPP_HIP_DEV_NO_QUAD_RUNS" not in knobs
        rec = out.setdefault(key, {"quad": int(quad), "jobs": 0, "points": collections.Counter()})
        rec["jobs"] += c
        rec["points"][n] += c
    for rec in out.values():
        rec["points"] = dict(rec["points"])
        rec["max_points"] = max(rec["points"])
    return out


# ---- the report -----------------------------------------------------------------------------------------------------------------

def _counts(text):
    return {} if text == "-" else {int(a): int(b) for a, b in (item.split("x") for item in text.split(","))}


def parse_report(err):
    """The "[schur report]" lines the tile analysis (csrc/schur_tile_tables.cpp) prints under SLAMPP_HIP_PLAN_TIMING."""
    rep = {"runs": {}, "tiles": None, "reduce": None, "routes": None, "lists_keep": None,
           "lines": [l for l in err.splitlines() if l.startswith("[schur report]") or l.startswith("[schur] of")]}
    for m in re.finditer(r"\[schur report\] runs: NT=(\d) diag=(\d) prefix=(\d) quad=(\d) jobs=(\d+) max_points=(\d+) points=(\S+)", err):
        nt, d, x, quad, jobs, max_points = (int(g) for g in m.groups()[:6])
        rep["runs"][(nt, d, x)] = {"quad": quad, "jobs": jobs, "max_points": max_points, "points": _counts(m.group(7))}
    m = re.search(r"\[schur report\] tiles: NL=(\d) tiles=(\d+) max_slots=(\d+) max_k=(\d+) max_points=(\d+)", err)
    if m:
        rep["tiles"] = dict(zip(("NL", "tiles", "max_slots", "max_k", "max_points"), (int(g) for g in m.groups())))
    m = re.search(r"\[schur report\] reduce: blocks=(\d+) longest=(\d+) off_diagonal=(\S+) diagonal=(\S+)", err)
    if m:
        rep["reduce"] = {"blocks": int(m.group(1)), "longest": int(m.group(2)), "off_diagonal": _counts(m.group(3)),
                         "diagonal": _counts(m.group(4))}
    m = re.search(r"\[schur report\] routes: runs=(\d+) prefix=(\d+) tiles=(\d+) lists=(\d+)", err)
    if m:
        rep["routes"] = dict(zip(("runs", "prefix", "tiles", "lists"), (int(g) for g in m.groups())))
    m = re.search(r"\[schur report\] the lists keep everything: rule=(\w+)", err)
    if m:
        rep["lists_keep"] = m.group(1)
    return rep


# ---- designed systems ---------------------------------------------------------------------------------------------------------

class Design:
    """The landmarks of one case, route by route.  ``run(cams, classes)``: a run on the camera list ``cams`` whose classes
    [(k, landmarks)], longest first, are seen by the first k of those cameras; ``tile`` / ``listed``: a landmark the case
    expects in a tile / on the contribution lists.  ``finish`` shuffles the landmarks (a run's members are then no
    neighbours in the system: the run kernel gathers them) unless the case depends on their order."""

    def __init__(self, dc):
        self.dc, self.lists, self.tags, self.chains = dc, [], [], []

    def run(self, cams, classes):
        cams = list(cams)
        assert all(k1 > k2 for (k1, _), (k2, _) in zip(classes, classes[1:])) and classes[0][0] == len(cams)
        assert len({nt_of(self.dc, k) for k, _ in classes}) == 1, "a chain stays inside one NT class"
        rid = len(self.chains)
        self.chains.append([k for k, n in classes for _ in range(n)])
        for k, n in classes:
            for _ in range(n):
                self.lists.append(cams[:k])
                self.tags.append(("run", rid, k))
        return rid

    def tile(self, cams, n=1):
        for _ in range(n):
            self.lists.append(list(cams))
            self.tags.append(("tile", -1, len(cams)))

    def listed(self, cams, n=1):
        for _ in range(n):
            self.lists.append(list(cams))
            self.tags.append(("list", -1, len(cams)))

    def finish(self, seed, shuffle=True):
        if shuffle:
            order = np.random.default_rng(seed).permutation(len(self.lists))
            self.lists = [self.lists[i] for i in order]
            self.tags = [self.tags[i] for i in order]
        return self

    def route_counts(self):
        n_run = sum(1 for t in self.tags if t[0] == "run")
        n_prefix = sum(len(c) for c in self.chains if len(set(c)) > 1)
        return {"runs": n_run, "prefix": n_prefix, "tiles": sum(1 for t in self.tags if t[0] == "tile"),
                "lists": sum(1 for t in self.tags if t[0] == "list")}

    def last_of_run(self, rid):
        """The last landmark of the last piece of run ``rid``: the last member (equal lists keep the system's order) of its
        shortest class."""
        k = min(self.chains[rid])
        return max(p for p, t in enumerate(self.tags) if t[:2] == ("run", rid) and t[2] == k)

    def last_of_tiles(self):
        """The last landmark of the last tile: tiles take their landmarks by (first camera, second camera), equal ones in
        the system's order."""
        def key(p):
            l = self.lists[p]
            return (l[0] if l else 0, l[1] if len(l) > 1 else (l[0] if l else 0), p)
        return max((p for p, t in enumerate(self.tags) if t[0] == "tile"), key=key)

    def some(self, route):
        """A landmark of the route from the middle of the system."""
        members = [p for p, t in enumerate(self.tags) if t[0] == route]
        return members[len(members) // 2]


@dataclasses.dataclass
class Case:
    design: object                       # dc -> Design
    mode: int                            # option schur_tiles
    knobs: dict = dataclasses.field(default_factory=dict)
    mult: int = 1                        # SLAMPP_HIP_DEV_RUN_PIECE_MULT of the knobs
    tiles: object = None                 # dc, dp -> the entries of the tile line the case expects (None: no tile launch)
    reduce: object = None                # dc -> {"off_diagonal" / "diagonal": {partial blocks: at least this many blocks}}
    lists_keep: str = None               # the rule, where the analysis leaves everything to the lists
    route: str = "run"                   # the route the changed and the indefinite landmark are on
    run_of_interest: int = -1            # ... the run (default: the last one designed)
    cams: tuple = (12, 45)               # cameras of the system
    seed: int = 0


class Fixture:
    """One case at one block size: the system, its dense Lambda and refined references, built once per process."""

    def __init__(self, case_name, case, dims):
        self.case, self.dims = case, dims
        dc, dp = dims
        self.design = case.design(dc)
        self.lam = build_system(self.design.lists, dc, dp, seed=1000 + case.seed, name=f"{case_name}_{dc}x{dp}")
        nc = self.lam.n_matrix_cut
        assert case.cams[0] <= nc <= case.cams[1], nc
        assert len(set(np.concatenate([np.asarray(l, dtype=np.int64) for l in self.design.lists]).tolist())) == nc, "a camera nobody sees"
        self.n_x = int(self.lam.cumsum[nc])
        rng = np.random.default_rng(2000 + case.seed)
        eta = self.lam.rhs
        eta_c, eta_l = eta.copy(), eta.copy()
        eta_c[self.n_x:] = 0.0                       # x_c = S^-1 eta_c: the blocks of S alone
        eta_l[:self.n_x] = 0.0                       # the U C^-1 l lanes and the partial right-hand sides alone
        self.B = np.stack([eta, eta_c, eta_l, rng.standard_normal(eta.shape[0])], axis=1)
        self._A = self._X = self._changed = None
        if case.route == "run":
            self.p_bad = self.design.last_of_run(range(len(self.design.chains))[case.run_of_interest])
            self.p_changed = self.p_bad
        elif case.route == "tile":
            self.p_bad = self.design.last_of_tiles()
            self.p_changed = self.design.some("tile")
        else:
            self.p_bad = self.p_changed = self.design.some("list")

    @property
    def A(self):
        if self._A is None:
            self._A = dense(self.lam)
        return self._A

    @property
    def X(self):
        if self._X is None:
            self._X = refined_solutions(self.A, self.B)
        return self._X

    @property
    def changed(self):
        """(the system with landmark p_changed moved, its own refined solution)."""
        if self._changed is None:
            lam2 = with_changed_landmark(self.lam, self.p_changed, np.random.default_rng(3000 + self.case.seed))
            self._changed = (lam2, refined_solutions(dense(lam2), lam2.rhs[:, None])[:, 0])
        return self._changed

    def expected_runs(self):
        jobs = collections.Counter()
        for chain in self.design.chains:
            jobs.update(run_jobs(self.dims[0], chain, self.case.mult))
        return launches_of(jobs, self.case.knobs)


_fixtures = {}


def fixture(cases, case_name, dims):
    key = (case_name, dims)
    if key not in _fixtures:
        _fixtures[key] = Fixture(case_name, cases[case_name], dims)
    return _fixtures[key]


# ---- the checks of one case ---------------------------------------------------------------------------------------------------

def check_report(fx, rep):
    """The report against what the case was designed to reach: a shape that is not there is a failure."""
    case = fx.case
    if case.lists_keep:
        assert rep["lists_keep"] == case.lists_keep and rep["routes"] is None and not rep["runs"], rep["lines"]
        return
    assert rep["lists_keep"] is None, rep["lines"]
    assert rep["runs"] == fx.expected_runs(), (rep["lines"], fx.expected_runs())
    assert rep["routes"] == fx.design.route_counts(), (rep["lines"], fx.design.route_counts())
    want = case.tiles(*fx.dims) if case.tiles else None
    if want is None:
        assert rep["tiles"] is None, rep["lines"]
    else:
        assert rep["tiles"] is not None and {k: rep["tiles"][k] for k in want} == want, (rep["lines"], want)
    if case.reduce:
        for where, lengths in case.reduce(fx.dims[0]).items():
            for n, n_blocks in lengths.items():
                assert rep["reduce"][where].get(n, 0) >= n_blocks, (where, n, rep["lines"])


def _held(x, ref, n_x, what):
    assert rel_inf(x, ref) < TOL, (what, rel_inf(x, ref))
    assert rel_inf(x[:n_x], ref[:n_x]) < TOL, (what, "cameras", rel_inf(x[:n_x], ref[:n_x]))
    assert rel_inf(x[n_x:], ref[n_x:]) < TOL, (what, "landmarks", rel_inf(x[n_x:], ref[n_x:]))


def analyzed(monkeypatch, capfd, fx, sparse, **options):
    """A handle with the case's mode and knobs, analyzed; the report of that analysis."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_Schur_HIP
    monkeypatch.setenv("SLAMPP_HIP_DEV", "1")
    for k, v in fx.case.knobs.items():
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    solver = CLinearSolver_Schur_HIP(schur_tiles=fx.case.mode, schur_sparse=sparse, **options)
    capfd.readouterr()
    assert solver.SymbolicDecomposition_Blocky(fx.lam)
    rep = parse_report(capfd.readouterr().err)
    monkeypatch.delenv("SLAMPP_HIP_PLAN_TIMING")
    return solver, rep


def run_case(monkeypatch, capfd, cases, case_name, dims, sparse):
    """Every check of one case on the reduced system written densely (``sparse`` = 0) or through p_dst / p_r into the inner
    sparse solver's arrays (1)."""
    from oracle import oracle_lib as O
    fx = fixture(cases, case_name, dims)
    lam, n_x, X = fx.lam, fx.n_x, fx.X
    # 1. reach: the report shows the launches, NL and routes the case is about
    solver, rep = analyzed(monkeypatch, capfd, fx, sparse, schur_keep=1)
    print("\n".join([f"{case_name} {dims} schur_tiles={fx.case.mode} schur_sparse={sparse} knobs={fx.case.knobs}"] + rep["lines"]))
    check_report(fx, rep)
    # 2. three right-hand sides: the system's own, one without a landmark part (S alone), one without a camera part (the
    # partial right-hand sides alone); the same call twice gives the same bits
    first = None
    for j, what in enumerate(("eta", "eta_c", "eta_l")):
        eta = fx.B[:, j].copy()
        assert solver.Solve_PosDef_Blocky(lam, eta)
        _held(eta, X[:, j], n_x, what)
        if j == 0:
            first = eta
    eta = fx.B[:, 0].copy()
    assert solver.Solve_PosDef_Blocky(lam, eta) and np.array_equal(eta, first)
    # 3. the W and C^-1 the route stored: a fourth right-hand side on the kept factor
    eta = fx.B[:, 3].copy()
    assert solver.Solve_Again(eta)
    _held(eta, X[:, 3], n_x, "Solve_Again")
    # 4. one landmark of the case's route is given an indefinite C; the next solve of the clean system is right
    bad = with_indefinite_landmark(lam, fx.p_bad)
    assert O.solve_schur(bad)[0] is False
    assert solver.Solve_PosDef_Blocky(bad, bad.rhs.copy()) is False
    eta = fx.B[:, 0].copy()
    assert solver.Solve_PosDef_Blocky(lam, eta)
    _held(eta, X[:, 0], n_x, "after the indefinite landmark")
    # 5. the incremental update of S for one named landmark of the route, against the changed system's own reference
    inc, rep_inc = analyzed(monkeypatch, capfd, fx, sparse, schur_incremental=2, profile=1)
    assert rep_inc["runs"] == rep["runs"] and rep_inc["routes"] == rep["routes"]
    eta = fx.B[:, 0].copy()
    assert inc.Solve_PosDef_Blocky(lam, eta)
    _held(eta, X[:, 0], n_x, "before the update")
    lam2, x2 = fx.changed
    inc.profile(reset=True)
    inc.Set_Changed_Landmarks([fx.p_changed])
    eta = lam2.rhs.copy()
    assert inc.Solve_PosDef_Blocky(lam2, eta)
    assert inc.profile().get("schur_update", (0, 0))[0] == 1          # (it was an update, not another assembly)
    _held(eta, x2, n_x, "incremental update")
    return fx, rep, first
