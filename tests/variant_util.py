"""Helpers of tests/test_sparse_variants_gpu.py: the small systems every schedule variant of the sparse block Cholesky is
pinned at, their plain high-precision references (never the library under test), the host code's gates restated over
plan() / stats() / profile(), and the one list of checks every variant goes through on one handle.

Nothing GPU-bound is imported at module level: the systems and references are built at first use and kept."""
import dataclasses
import functools

import numpy as np

from slam_plus_plus_amd import synth

TOL = 1e-10                       # the project's bound on ||x - x_ref||_inf / ||x_ref||_inf
L_TOL = 1e-11                     # ... and on max|L - L_ref| / max|L_ref| (test_factorize_returns_the_cholesky_factor)
WIDE_CHUNK, WIDE_NR, WIDE_NP = 8, 32, 48        # sparse_kernels.h:174: what a packaged column of a wide stage may hold
SIMT_MAX_PROG, SIMT_MAX_TABLE_BYTES = 4096, 40960   # sparse_records.cpp: SIMT_MAX_PROG, SIMT_MAX_TABLE_BYTES
PLAN_OPTIONS = {"subtree_size": 4, "leaf_size": 1, "dense_top_nb": 0}   # ~n/4 leaf tasks, six or more stages, no dense top
ALPHAS = (0.0, 0.5, 1e-3)                       # the batch members: Lambda + alpha I
ALPHAS_8 = (0.0, 0.5, 1e-3, 7.0, 1e-6, 0.25, 2.0, 0.03)
MIXED_SEED = 1012                                # random_system(): 150 <= n <= 400, block sizes 2 .. 8 mixed (asserted below)


def rel_inf(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def damped(lam, alpha):
    """Lambda + alpha I on a copy."""
    off = lam.block_value_offsets()
    v = lam.values.copy()
    for j in range(lam.n_bcols):
        k = int(lam.bcol_ptr[j + 1] - 1)
        d = int(lam.cumsum[j + 1] - lam.cumsum[j])
        v[off[k]:off[k + 1]].reshape(d, d)[...] += alpha * np.eye(d)
    return dataclasses.replace(lam, values=v)


def with_bad_column(lam, j_old):
    """A copy with 1e4 I subtracted from the diagonal block of (the caller's) block column j_old."""
    off = lam.block_value_offsets()
    k = int(lam.bcol_ptr[j_old + 1] - 1)
    d = int(lam.cumsum[j_old + 1] - lam.cumsum[j_old])
    v = lam.values.copy()
    v[off[k]:off[k + 1]] -= 1e4 * np.eye(d).ravel()
    return dataclasses.replace(lam, values=v)


def hub_chain(n=300, d=6, seed=71):
    """The package-limit system: a 6-dof pose chain with loop closures, one hub vertex (number n) joined to the 60 poses
    10 .. 69, a banded stretch (poses 180 .. 259 also see their second and third successors) and three side branches
    (a vertex with two paths of two hanging off it).  The hub's column collects more row entries than a package of a wide
    stage holds, but nested dissection puts it near the root, in a stage of few tasks; the band puts columns over the limits
    into the crowded stages right above the leaves as well, and the branch vertices are the columns with next to no updates."""
    rng = np.random.default_rng(seed)
    ci = np.arange(n - 1)
    ends = np.arange(50, n, 50)
    li = ends - rng.integers(26, 51, size=len(ends))
    band = np.arange(180, 260)
    ei = [ci, li, np.arange(10, 70), band, band]
    ej = [ci + 1, ends, np.full(60, n), band + 2, band + 3]
    nv = n + 1
    for a in (100, 140, 290):
        q = nv
        nv += 5
        ei.append(np.array([a, q, q + 1, q, q + 3]))
        ej.append(np.array([q, q + 1, q + 2, q + 3, q + 4]))
    return synth._assemble_pose_graph(nv, d, np.concatenate(ei), np.concatenate(ej), rng, 0.02, 100.0, f"hub_chain_n{n}")


def _mixed():
    from test_sparse_gpu import random_system
    lam, _ = random_system(MIXED_SEED)
    dims = np.diff(lam.cumsum).tolist()
    assert 150 <= lam.n_bcols <= 400 and len(set(dims)) > 1
    return lam


SYSTEMS = {
    "chain3": lambda: synth.pose_chain(n=612, d=3, seed=62),
    "chain6": lambda: synth.pose_chain(n=612, d=6, seed=62),
    "chain7": lambda: synth.pose_chain(n=610, d=7, seed=63),  # (612 / 610 poses: a leaf shape of 65 / 66 tasks)
    "sphere": lambda: synth.sphere(12, 12),
    "hub": hub_chain,
    "mixed": _mixed,
}


def refined_solution(lam):
    """x of Lambda x = eta: sparse LU in fp64, then two steps of iterative refinement with the residual eta - Lambda x
    accumulated in long double over the triplets of the blocks (both triangles)."""
    import scipy.sparse.linalg as sla
    A = lam.to_scipy().tocsc()
    lu = sla.splu(A)
    coo = A.tocoo()
    ld = np.longdouble
    data, row, col = coo.data.astype(ld), coo.row, coo.col
    b = lam.rhs.astype(ld)
    x = lu.solve(lam.rhs)
    for _ in range(2):
        r = b.copy()
        np.subtract.at(r, row, data * x.astype(ld)[col])
        x = x + lu.solve(r.astype(np.float64))
    return x


class System:
    """One system with its references, built once per process."""

    def __init__(self, name):
        from oracle import oracle_lib as O
        self.name = name
        self.lam = SYSTEMS[name]()
        self.dims = np.diff(self.lam.cumsum).astype(np.int64)
        self.uniform = len(set(self.dims.tolist())) == 1
        self.d = int(self.dims[0]) if self.uniform else 0
        self.x_ref = refined_solution(self.lam)
        ok, x_oracle, _ = O.solve_sparse(self.lam)      # the CPU oracle and the refined solution agree: a disagreement
        assert ok and rel_inf(x_oracle, self.x_ref) < TOL   # on the GPU does not come from the reference
        self._members, self._factors, self._refused = {}, {}, {}

    def member(self, alpha):
        """(Lambda + alpha I, its refined solution for the right-hand side eta)."""
        if alpha not in self._members:
            m = damped(self.lam, alpha) if alpha else self.lam
            self._members[alpha] = (m, refined_solution(m) if alpha else self.x_ref)
        return self._members[alpha]

    def oracle_refuses(self, j_old):
        from oracle import oracle_lib as O
        if j_old not in self._refused:
            bad = damped(self.lam, j_old[1]) if isinstance(j_old, tuple) else with_bad_column(self.lam, j_old)
            self._refused[j_old] = O.solve_sparse(bad)[0] is False
        return self._refused[j_old]

    def oracle_refuses_damping(self, alpha=-40.0):
        return self.oracle_refuses(("damped", alpha))

    def factor_reference(self, st):
        """numpy's Cholesky factor of the dense Lambda permuted as the factor structure ``st`` says, checked once to be zero
        outside the blocks of that structure (so that comparing block by block compares everything)."""
        key = st["perm"].tobytes()
        if key not in self._factors:
            A = self.lam.to_scipy().toarray()
            cs_old = self.lam.cumsum
            idx = np.concatenate([np.arange(cs_old[o], cs_old[o + 1]) for o in st["perm"]])
            Lref = np.linalg.cholesky(A[np.ix_(idx, idx)])
            cs = np.concatenate([[0], np.cumsum(st["dim"])]).astype(np.int64)
            outside = np.abs(Lref)
            for j in range(len(st["dim"])):
                for k in range(st["lptr"][j], st["lptr"][j + 1]):
                    i = st["lrow"][k]
                    outside[cs[i]:cs[i + 1], cs[j]:cs[j + 1]] = 0.0
            assert outside.max() == 0.0
            if len(self._factors) >= 2:                  # (nested dissection and the natural order: nothing else is asked for)
                self._factors.clear()
            self._factors[key] = (Lref, cs, float(np.abs(Lref).max()))
        return self._factors[key]


@functools.lru_cache(maxsize=None)
def system(name):
    return System(name)


def check_factor(sysrec, st, l_values):
    """Every block of the returned factor against the dense Cholesky factor; exact zeros above the diagonal."""
    Lref, cs, scale = sysrec.factor_reference(st)
    dim, lptr, lrow, loff = st["dim"], st["lptr"], st["lrow"], st["loff"]
    worst, upper = 0.0, 0.0
    for j in range(len(dim)):
        dj = int(dim[j])
        for k in range(lptr[j], lptr[j + 1]):
            i = int(lrow[k])
            blk = l_values[loff[k]:loff[k] + int(dim[i]) * dj].reshape(dj, int(dim[i])).T
            worst = max(worst, float(np.abs(blk - Lref[cs[i]:cs[i + 1], cs[j]:cs[j + 1]]).max()))
            if k == lptr[j]:
                assert i == j
                upper = max(upper, float(np.abs(np.triu(blk, 1)).max()))
    assert upper == 0.0
    assert worst < L_TOL * scale, (worst / scale)


# ---- the plan as the host code sees it ----------------------------------------------------------------------------------------

def stage_tasks(plan, s):
    return int(plan["stage_ptr"][s + 1] - plan["stage_ptr"][s])


def stage_columns(plan, s):
    """The (new-order) columns stage s eliminates: stage_ptr -> task_ptr -> task_cols."""
    t0, t1 = plan["stage_ptr"][s], plan["stage_ptr"][s + 1]
    return plan["task_cols"][plan["task_ptr"][t0]:plan["task_ptr"][t1]]


def column_counts(plan, j):
    """(nb, nr, np) of scheduled column j as fill_column_records() packs them (sparse_records.cpp)."""
    lptr, rptr, pptr = plan["lptr"], plan["rptr"], plan["pptr"]
    return int(lptr[j + 1] - lptr[j]), int(rptr[j + 1] - rptr[j]), int(pptr[lptr[j + 1]] - pptr[lptr[j] + 1])


def bottom_stages(plan, wide_min_tasks):
    """n_bottom_stages as count_bottom_stages() counts them (sparse_records.cpp)."""
    n_stages, n = len(plan["stage_ptr"]) - 1, 1
    while n < n_stages and stage_tasks(plan, n) > wide_min_tasks:
        n += 1
    return n


def task_shapes(plan, s, width):
    """The tasks of stage s grouped by shape as build_simt_tables() groups them (sparse_records.cpp: Simt_Task_Program(), Group_Simt_Shapes()): a shape is the task's
    program, its operands numbered in order of first use.  Returns [(number of tasks, fits the lane-per-task kernel)]."""
    lptr, lrow, pptr, pa, pb, rptr, rblk = (plan[k] for k in ("lptr", "lrow", "pptr", "pa", "pb", "rptr", "rblk"))
    blk_col = np.repeat(np.arange(len(lptr) - 1), np.diff(lptr))
    groups = {}
    for t in range(plan["stage_ptr"][s], plan["stage_ptr"][s + 1]):
        cols = plan["task_cols"][plan["task_ptr"][t]:plan["task_ptr"][t + 1]].tolist()
        ops, ys, prog, n_blocks, n_prog = {}, {}, [], 0, 4
        for j in cols:
            nb, nr = int(lptr[j + 1] - lptr[j]), int(rptr[j + 1] - rptr[j])
            body, touch = [], set()
            for e in range(rptr[j], rptr[j + 1]):
                blk = int(rblk[e])
                body += [ops.setdefault(blk, len(ops)), ys.setdefault(int(blk_col[blk]), len(ys))]
                touch.add(body[-2])
            for k in range(lptr[j] + 1, lptr[j + 1]):
                body.append(int(pptr[k + 1] - pptr[k]))
                for e in range(pptr[k], pptr[k + 1]):
                    body += [ops.setdefault(int(pa[e]), len(ops)), ops.setdefault(int(pb[e]), len(ops))]
                    touch.update(body[-2:])
            prog += [nb, nr] + body
            n_blocks += nb
            n_prog += 3 + len(touch) + len(body)
        tail = [cols.index(int(lrow[k])) if int(lrow[k]) in cols else -1 for j in cols for k in range(lptr[j] + 1, lptr[j + 1])]
        n_fields = 4 * len(cols) + n_blocks + len(ops) + len(ys)
        fits = n_prog + len(tail) <= SIMT_MAX_PROG and n_fields <= SIMT_MAX_TABLE_BYTES // (8 * width)
        key = (tuple(prog), tuple(tail))
        n, f = groups.get(key, (0, True))
        groups[key] = (n + 1, f and fits)
    return list(groups.values())


@dataclasses.dataclass
class Reach:
    """What a reach predicate looks at: the analysis of the handle under test."""
    sysrec: System
    options: dict
    knobs: dict
    plan: dict
    stats: dict

    def opt(self, name, default):
        return int(self.options.get(name, default))

    def knob(self, name, default):
        return int(self.knobs.get(name, default))

    @property
    def n_stages(self):
        return len(self.plan["stage_ptr"]) - 1

    @property
    def n_bottom(self):
        return int(self.stats["n_bottom_stages"])

    @property
    def fixed_dim(self):
        return self.sysrec.uniform and self.sysrec.d in (3, 6, 7)

    def simt_stage_count(self):
        """Stages the lane-per-task kernels take (build_simt_tables() in sparse_records.cpp: its early returns, the condition of its stage loop, and no chunk at all): option simt = 1, one of
        the fixed block sizes, s < n_bottom_stages and s < simt_stages, and tasks that fit the kernel's tables."""
        if self.opt("simt", -1) != 1 or not self.fixed_dim:
            return 0
        n = min(self.n_bottom, self.n_stages, self.opt("simt_stages", 1))
        width = self.opt("simt_width", 32)
        return n if any(f for s in range(n) for _, f in task_shapes(self.plan, s, width)) else 0

    def panels_on(self):
        return self.opt("panel", 1) != 0 and self.fixed_dim       # b_Panel_Pass(), sparse_records.cpp: t_opt.n_panel && b_Package_Dim(P)

    def panel_stages(self):
        """Stages launched as panels (b_leaf_panels and b_panel_stage in CPanelPass::Run(), sparse_records.cpp; sparse_enqueue.hip:103, 108): the separator stages, and the
        leaf stage where the lane-per-task kernel is not asked for and the leaf tasks are at most 512."""
        if not self.panels_on():
            return []
        leaf = self.opt("simt", -1) <= 0 and stage_tasks(self.plan, 0) <= 512
        return ([0] if leaf else []) + list(range(self.n_bottom, self.n_stages))


# the reach predicates: each restates the gate the host code evaluates, names its source line and asserts it ------------------

def reach_wide(r):
    """Gate 1, sparse_enqueue.hip:105: s > 0 && s < n_bottom_stages && dplan.task_pkg (packages exist for one fixed block size,
    build_column_packages(): b_Package_Dim(P)), for a stage the lane-per-task kernel has not taken (sparse_enqueue.hip:91)."""
    assert r.n_bottom >= 2 and r.n_bottom == bottom_stages(r.plan, r.opt("wide_min_tasks", 8192))
    assert r.fixed_dim
    assert max(r.simt_stage_count(), 1) < r.n_bottom


def reach_wide_packages(r):
    """Gate 1, both sides of factor_stage_kernel's cd.nb <= CH && cd.nr <= NR && cd.np <= NP (sparse_kernels.hip:135, 150): the
    wide stages hold a column over the limits (the general path) and columns within them whose ne = nr + np covers the
    smallest value, a value below BATCH = 4 and every residue mod 4 (the tails of the W == 1 loop, sparse_kernels.hip:207-255)."""
    reach_wide(r)
    counts = [column_counts(r.plan, int(j)) for s in range(max(r.simt_stage_count(), 1), r.n_bottom) for j in stage_columns(r.plan, s)]
    fits = [nb <= WIDE_CHUNK and nr <= WIDE_NR and np_ <= WIDE_NP for nb, nr, np_ in counts]
    assert not all(fits) and any(fits)
    ne = sorted({nr + np_ for (nb, nr, np_), f in zip(counts, fits) if f})
    assert ne[0] < 4 and {e % 4 for e in ne} == {0, 1, 2, 3}, ne


def reach_wide_mixed(r):
    """Gate 2, sparse_enqueue.hip:105 is false without packages (!P.uniform_dim: b_Package_Dim(P) in build_column_packages(), dplan.task_pkg in Analyze_Sparse()) and the stage falls
    through to launch_factor_stage(..., s < n_bottom_stages) at sparse_enqueue.hip:111 with s > 0."""
    assert r.n_bottom >= 2 and r.n_bottom == bottom_stages(r.plan, r.opt("wide_min_tasks", 8192))
    assert not r.sysrec.uniform and len(set(r.sysrec.dims.tolist())) > 1


def reach_simt(r):
    """Gate 3, sparse_enqueue.hip:52, 91 and simt_kernel.hip:392-399: the leaf stage by factor_simt_kernel<D, W, LPT, StoreLinv>;
    a shape with more members than one wave and a count that is no multiple of 16 runs the chunk tail of every width."""
    assert r.simt_stage_count() >= 1
    width = r.opt("simt_width", 32)
    assert width in (16, 32, 64)
    assert any(f and n > 64 and n % 16 != 0 for n, f in task_shapes(r.plan, 0, width))
    pairs = r.knob("SLAMPP_HIP_DEV_SIMT_PAIRS", -1)
    assert pairs in (0, 1)                                     # LPT = 2 iff pairs, even D and W <= 32; else LPT = 1
    r.lanes_per_task = 2 if pairs == 1 and r.sysrec.d % 2 == 0 and width <= 32 else 1


def reach_simt_backward(r):
    """StoreLinv = false and backward_simt_kernel, sparse_enqueue.hip:39-41, 93, 173: simt_backward = 1 on lane-per-task stages
    (the handle's own vectors are 16-byte aligned); nothing has asked for the leaf inverses on a fresh handle."""
    reach_simt(r)
    assert r.opt("simt_backward", -1) == 1


def reach_simt_stages(r):
    """Gate 4, the stage loop of build_simt_tables(): s < n_bottom_stages && s < n_simt_stages for a stage above the leaves."""
    assert r.n_bottom >= 2 and r.opt("simt_stages", 1) >= 2
    assert r.simt_stage_count() >= 2
    width = r.opt("simt_width", 32)
    assert any(f for s in range(1, r.simt_stage_count()) for _, f in task_shapes(r.plan, s, width))


def reach_panel_waves(waves):
    def reach(r):
        """Gate 7, n_stage_waves in CPanelPass::Decide_Stage(): a panel stage with more tasks than SLAMPP_HIP_DEV_PANEL_W2_MIN runs two waves a task,
        one with more than _W4_MIN (and not more than _W2_MIN) four."""
        w4, w2 = r.knob("SLAMPP_HIP_DEV_PANEL_W4_MIN", 512), r.knob("SLAMPP_HIP_DEV_PANEL_W2_MIN", 1024)
        got = {2 if stage_tasks(r.plan, s) > w2 else 4 if stage_tasks(r.plan, s) > w4 else 8 for s in r.panel_stages()}
        assert waves in got, got
    return reach


def reach_panel_no_riders(r):
    """Gate 7, n_ride_max_fresh in CPanelPass::Decide_Stage() (panel_ride[s] = n_max_fresh <= n_ride_max_fresh): with SLAMPP_HIP_DEV_PANEL_RIDE_FRESH = 0 a stage's updates ride in the launch below only
    if the stage right below contributes nothing; there are panel stages on top of panel stages for that to matter."""
    assert r.knob("SLAMPP_HIP_DEV_PANEL_RIDE_FRESH", 96) == 0
    ps = r.panel_stages()
    assert sum(1 for s in ps if s > 0 and s - 1 in ps) >= 2


def reach_handup_narrow(r):
    """Gate 7, b_hand_up_stage in CPanelPass::Decide_Stage() (n_handup_max_tasks): hand-ups only from stages of at most SLAMPP_HIP_DEV_HANDUP_MAX_TASKS tasks -- the plan has
    panel stages on either side of the line."""
    n_max = r.knob("SLAMPP_HIP_DEV_HANDUP_MAX_TASKS", 1 << 30)
    ps = [s for s in r.panel_stages() if s > 0 and s - 1 in r.panel_stages()]
    assert any(stage_tasks(r.plan, s - 1) <= n_max for s in ps) and any(stage_tasks(r.plan, s - 1) > n_max for s in ps)


def reach_task_caps(r):
    """Gate 7, plan.cpp:1109, 1346-1347: a slice of the tree is cut at SLAMPP_HIP_DEV_TASK_MAX_COLS columns / _TASK_MAX_BLOCKS blocks."""
    n_cols = r.knob("SLAMPP_HIP_DEV_TASK_MAX_COLS", 8)
    n_blocks = r.knob("SLAMPP_HIP_DEV_TASK_MAX_BLOCKS", 96)
    tp, lptr = r.plan["task_ptr"], r.plan["lptr"]
    sizes, tall = [], []
    for s in range(r.n_bottom, r.n_stages):
        for t in range(r.plan["stage_ptr"][s], r.plan["stage_ptr"][s + 1]):
            cols = r.plan["task_cols"][tp[t]:tp[t + 1]]
            sizes.append((len(cols), int(sum(lptr[j + 1] - lptr[j] for j in cols))))
            tall.append(len(cols) > 1)
    assert sizes and all(c <= n_cols and (c == 1 or b <= n_blocks) for c, b in sizes)
    assert any(c == n_cols for c, _ in sizes) or n_blocks < 96     # the cap binds: some slice is cut right at it
    assert any(tall) or n_blocks < 96


def reach_subtree_v1(r):
    """Gate 7, sparse_kernels.hip:653-657 behind sparse_enqueue.hip:111: the leaf stage by launch_factor_stage(b_bottom_stage)
    with SLAMPP_HIP_DEV_SUBTREE_V1 set -- neither lane-per-task (simt = 0) nor panels (few leaf tasks would go to the panel
    kernel, b_leaf_panels in CPanelPass::Run())."""
    assert "SLAMPP_HIP_DEV_SUBTREE_V1" in r.knobs and r.opt("simt", -1) == 0
    assert 0 not in r.panel_stages() and r.fixed_dim


def reach_batch(r):
    """Gate 5, capi.hip: slampp_hip_factor_solve_batch_device_async: K > 1 members in one pass of launches (blockIdx.y) needs no
    dense top, no regrouped values and aligned bases / even strides; the test passes those."""
    assert r.plan["dense_dim"] == 0 and int(r.sysrec.dims.max()) <= 8


# ---- the checks of one variant ---------------------------------------------------------------------------------------------------

def _pick_column(r, stage):
    """A column (in the caller's numbering) that stage ``stage`` eliminates: the middle one."""
    cols = stage_columns(r.plan, stage)
    return int(r.plan["perm"][int(cols[len(cols) // 2])])


def _batch(solver, sysrec, alphas, odd, expect=None):
    """The members Lambda + alpha I with right-hand sides (k + 1) eta in one batch call; every good member against its own
    refined reference."""
    import torch
    lam = sysrec.lam
    K = len(alphas)
    sv, sr = lam.values.shape[0] + 6, lam.n_scalars + 6
    sv += (1 - sv % 2) if odd else sv % 2
    sr += (1 - sr % 2) if odd else sr % 2
    vals = torch.zeros(K * sv, dtype=torch.float64, device="cuda")
    rhs = torch.zeros(K * sr, dtype=torch.float64, device="cuda")
    members = [damped(lam, a) if a < 0 else sysrec.member(a)[0] for a in alphas]
    for k, m in enumerate(members):
        vals[k * sv:k * sv + m.values.shape[0]] = torch.from_numpy(m.values).cuda()
        rhs[k * sr:k * sr + m.n_scalars] = torch.from_numpy((k + 1.0) * m.rhs).cuda()
    torch.cuda.synchronize()
    assert vals.data_ptr() % 16 == 0 and rhs.data_ptr() % 16 == 0
    solver.factor_solve_batch_device_async(K, vals.data_ptr(), sv, rhs.data_ptr(), sr)
    assert solver.sync_batch(K) == (expect or [True] * K)
    x = rhs.cpu().numpy()
    for k, a in enumerate(alphas):
        if a >= 0:
            assert rel_inf(x[k * sr:k * sr + lam.n_scalars], (k + 1.0) * sysrec.member(a)[1]) < TOL, (k, a, odd)


def run_variant(monkeypatch, name, options, knobs, reaches, stage_of=None, natural=False, alphas=ALPHAS, profile_phase=None):
    """Every check of one schedule variant on one handle: reach, factor, solves, batch, failure surface.

    ``reaches``: the predicates above; ``stage_of(r)``: the stage whose kernel the variant is about (the failure is planted in
    a column it eliminates; default: the leaf stage); ``profile_phase``: a phase that must have run (option profile = 2)."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    sysrec = system(name)
    lam, x_ref = sysrec.lam, sysrec.x_ref
    options = dict(PLAN_OPTIONS, **options)
    solver = CLinearSolver_HIP(**options)
    # 1. reach
    assert solver.SymbolicDecomposition_Blocky(lam)
    r = Reach(sysrec, options, dict(knobs), solver.plan(), solver.stats())
    for reach in reaches:
        reach(r)
    reach_batch(r)
    # 2. the factor, block by block (nested dissection; the natural order on a handle of its own)
    ok, st, l_values = solver.factorize(lam)
    assert ok
    assert not np.array_equal(st["perm"], np.arange(lam.n_bcols))
    check_factor(sysrec, st, l_values)
    if natural:
        ok, st, l_values = CLinearSolver_HIP(**dict(options, natural_order=1)).factorize(lam)
        assert ok and np.array_equal(st["perm"], np.arange(lam.n_bcols))
        check_factor(sysrec, st, l_values)
    # 3. solves: cold, warm with another right-hand side, the kept factor (the forward kernel; inverses fixed up late)
    solver.set_option("profile", 2)
    solver.profile(reset=True)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, eta) and rel_inf(eta, x_ref) < TOL
    if profile_phase:
        assert solver.profile().get(profile_phase, (0, 0.0))[0] > 0, solver.profile()
    assert solver.stats()["n_bottom_stages"] == r.n_bottom and np.array_equal(solver.plan()["task_cols"], r.plan["task_cols"])
    solver.set_option("profile", 0)
    eta = 2.0 * lam.rhs
    assert solver.Solve_PosDef_Blocky(lam, eta) and rel_inf(eta, 2.0 * x_ref) < TOL
    eta = -lam.rhs
    assert solver.Solve_Again(eta) and rel_inf(eta, -x_ref) < TOL
    # 4. batches: even member strides (one pass of launches), odd ones (member by member), one member not positive definite
    _batch(solver, sysrec, alphas, odd=False)
    _batch(solver, sysrec, alphas[:3], odd=True)
    assert sysrec.oracle_refuses_damping()
    _batch(solver, sysrec, (alphas[0], -40.0, alphas[2]), odd=False, expect=[True, False, True])
    # 5. a failure inside this variant's stage surfaces, and the flag is clean afterwards
    j_old = _pick_column(r, stage_of(r) if stage_of else 0)
    assert sysrec.oracle_refuses(j_old)
    bad = with_bad_column(lam, j_old)
    assert solver.Solve_PosDef_Blocky(bad, bad.rhs.copy()) is False
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta) and rel_inf(eta, x_ref) < TOL
    return r


def run_misaligned(monkeypatch, name, options):
    """Gate 6, sparse_enqueue.hip:41, 52-53, 186-187: device pointers that are 8-byte aligned only.  With an even block size the
    lane-per-task kernels step aside (16-byte loads and stores) and the wave-per-task backward kernel needs the inverses the
    lane-per-task factorization did not store; with an odd one nothing changes."""
    import torch
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    sysrec = system(name)
    lam, x_ref = sysrec.lam, sysrec.x_ref
    options = dict(PLAN_OPTIONS, **options)
    nv, ns = lam.values.shape[0], lam.n_scalars
    vals = torch.zeros(nv + 2, dtype=torch.float64, device="cuda")
    rhs = torch.zeros(ns + 2, dtype=torch.float64, device="cuda")
    assert vals.data_ptr() % 16 == 0 and rhs.data_ptr() % 16 == 0
    for shift in ((1, 0), (0, 1), (1, 1)):           # values, right-hand side, both 8-byte aligned only
        solver = CLinearSolver_HIP(**options)
        assert solver.SymbolicDecomposition_Blocky(lam)
        r = Reach(sysrec, options, {}, solver.plan(), solver.stats())
        assert r.simt_stage_count() >= 1            # an aligned solve takes the lane-per-task kernels: sparse_enqueue.hip:52
        for shift_v, shift_r in ((0, 0), shift):    # aligned first: with simt_backward = 1 that factorization stores no inverses
            vals[shift_v:shift_v + nv] = torch.from_numpy(lam.values).cuda()
            rhs[shift_r:shift_r + ns] = torch.from_numpy(lam.rhs).cuda()
            torch.cuda.synchronize()
            solver.factor_solve_device_async(vals.data_ptr() + 8 * shift_v, rhs.data_ptr() + 8 * shift_r)
            assert solver.sync() is True
            assert rel_inf(rhs[shift_r:shift_r + ns].cpu().numpy(), x_ref) < TOL, (shift_v, shift_r)
        eta = -lam.rhs
        assert solver.Solve_Again(eta) and rel_inf(eta, -x_ref) < TOL, shift
