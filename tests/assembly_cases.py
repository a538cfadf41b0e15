"""Small designed systems for the device Lambda / eta assembly (csrc/assembly.hip), one per route of its dispatch, with a
long-double reference and a derived tolerance.  Used by tests/test_assembly_tables_sanitizers.py (CPU: the host builder's
tables, the branches each case reaches, the reference's own error) and tests/test_assembly_routes_gpu.py (the kernels).
Nothing GPU-bound is imported here.

Reference (never the library, never the C oracle), in numpy.longdouble, for one edge set:
    off-diagonal block (min, max)  = sum w J0^T Sigma^-1 J1, transposed where v0 > v1
    diagonal blocks                = sum w J^T Sigma^-1 J
    eta of vertex 0                = sum w^2 J0^T Sigma^-1 e     (the reference's double weight)
    eta of vertex 1                = sum w J1^T Sigma^-1 e
    the anchor                     += U^T U and the unary error
and beside every entry the same sum over absolute values, S_abs.

Tolerance, per entry, derived and not measured: |got - ref| <= (ne + 2 rd + 4 [+ d on the anchored vertex]) 2^-53 S_abs,
ne the number of edges of that entry's block.  An entry is a sum of ne terms, each two nested rd-term dot products
(J^T (Sigma^-1 J) or (J^T Sigma^-1) J) times w or w^2: a dot product of k terms computed in any order, with or without FMA,
is off by at most k 2^-53 sum|a||b| to first order, two nested ones by 2 rd, the weight adds up to two roundings, the sum
over the edges ne more, and two are left for the second-order terms; the anchor's U^T U is a d-term dot product more.
``fp64_restatement`` is the same arithmetic in numpy float64: the host test asserts it stays under half the bound, which
keeps the bound one on the kernels and not on the reference.

Accumulation onto what the arrays hold: the held values are drawn no larger than S_abs entry by entry (uniform in
(-1, 1) S_abs; in (-1, 1) where no edge contributes), and the bound is widened by one rounding of the sum,
2^-53 |held + ref|."""
import dataclasses
from typing import Optional

import numpy as np

from slam_plus_plus_amd import synth

LD = np.longdouble
U53 = 2.0 ** -53


@dataclasses.dataclass
class Case:
    name: str
    dims: np.ndarray
    v0: np.ndarray
    v1: np.ndarray
    rd: int
    groups: Optional[int]          # option "assembly_groups"; None: the library's default
    anchor: int
    reached: frozenset             # branches of the host builder this case must reach
    not_reached: frozenset = frozenset()
    extra_pairs: tuple = ()        # off-diagonal blocks of Lambda that no edge of the set touches
    anchor_route: str = ""         # route the anchored vertex must take: group, long, small, plain
    seed: int = 0

    def structure(self):
        ex = np.array(self.extra_pairs, dtype=np.int64).reshape(-1, 2)
        return synth.structure_from_edges(self.dims, np.concatenate([self.v0, ex[:, 0]]), np.concatenate([self.v1, ex[:, 1]]))

    def edge_set(self):
        """synth.random_edge_set's recipe (Sigma^-1 = A A^T + c I: not diagonal), with an anchor factor that is not symmetric."""
        es = synth.random_edge_set(self.dims, self.v0, self.v1, rd=self.rd, seed=self.seed + 1, robust=True, anchor=self.anchor)
        rng = np.random.default_rng(self.seed + 77)
        d = int(self.dims[self.anchor])
        es.unary_factor = np.eye(d) * 100.0 + rng.standard_normal((d, d))
        es.unary_error = 0.1 * rng.standard_normal(d)
        return es


def case_text(case: Case) -> str:
    """One case of the driver's cases file (tests/assembly_tables_driver.cpp): name, n, n_edges, n_extra, rd, groups
    (-1: the default); then the dimensions, v0, v1 and the extra pairs."""
    ex = np.array(case.extra_pairs, dtype=np.int64).reshape(-1, 2)
    head = "case %s %d %d %d %d %d" % (case.name, len(case.dims), len(case.v0), len(ex), case.rd,
                                       -1 if case.groups is None else case.groups)
    return "\n".join([head] + [" ".join(str(int(x)) for x in a) for a in (case.dims, case.v0, case.v1, ex.reshape(-1))]) + "\n"


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------

def reference(lam, es, weights=True, unary=True, dtype=LD):
    """(values, eta, S_abs of values, S_abs of eta, bound of values, bound of eta, touched values mask, touched eta mask) for
    the edge set on lam's structure; ``dtype`` numpy.longdouble for the reference, numpy.float64 for the restatement."""
    cs, ptr, brow = lam.cumsum, lam.bcol_ptr, lam.brow_idx
    n = len(cs) - 1
    off = lam.block_value_offsets()
    J0, J1, S, e = (np.asarray(a, dtype=dtype) for a in (es.J0, es.J1, es.sigma_inv, es.err))
    ne, rd = es.n_edges, es.rd
    w = np.asarray(es.weight, dtype=dtype) if (weights and es.weight is not None) else np.ones(ne, dtype=dtype)
    # J[e, c, a] is J(a, c); S[e, b, a] is Sigma^-1(a, b)
    # (two nested rd-term dot products, as the bound counts them: a three-operand einsum would sum rd^2 products in a row)
    def quad(A, B, wt, S=S):
        return np.einsum("eia,eja->eij", A, np.einsum("eba,ejb->eja", S, B)) * wt[:, None, None]

    def rhs(A, wt, S=S, e=e):
        return np.einsum("eia,ea->ei", A, np.einsum("eba,eb->ea", S, e)) * wt[:, None]
    aJ0, aJ1, aS, ae = np.abs(J0), np.abs(J1), np.abs(S), np.abs(e)

    def quad_abs(A, B, wt):
        return quad(A, B, wt, aS)

    def rhs_abs(A, wt):
        return rhs(A, wt, aS, ae)
    values, v_abs = np.zeros(lam.values.shape[0], dtype=dtype), np.zeros(lam.values.shape[0], dtype=dtype)
    eta, e_abs = np.zeros(int(cs[-1]), dtype=dtype), np.zeros(int(cs[-1]), dtype=dtype)
    v_ne, e_ne = np.zeros(lam.values.shape[0]), np.zeros(int(cs[-1]))
    H01, A01 = quad(J0, J1, w), quad_abs(aJ0, aJ1, w)
    H00, A00 = quad(J0, J0, w), quad_abs(aJ0, aJ0, w)
    H11, A11 = quad(J1, J1, w), quad_abs(aJ1, aJ1, w)
    y0, b0 = rhs(J0, w * w), rhs_abs(aJ0, w * w)
    y1, b1 = rhs(J1, w), rhs_abs(aJ1, w)
    blk = {}
    for c in range(n):
        for k in range(int(ptr[c]), int(ptr[c + 1])):
            blk[(int(brow[k]), c)] = k
    for i in range(ne):          # in edge order, as every kernel's lists are
        a, b = int(es.v0[i]), int(es.v1[i])
        k = blk[(min(a, b), max(a, b))]
        h, ha = (H01[i], A01[i]) if a < b else (H01[i].T, A01[i].T)       # rows x cols of the stored block
        sl = slice(int(off[k]), int(off[k + 1]))
        values[sl] += h.T.reshape(-1)                                       # column-major
        v_abs[sl] += ha.T.reshape(-1)
        v_ne[sl] += 1
        for v, hd, hda, y, ya in ((a, H00[i], A00[i], y0[i], b0[i]), (b, H11[i], A11[i], y1[i], b1[i])):
            k = blk[(v, v)]
            sl = slice(int(off[k]), int(off[k + 1]))
            values[sl] += hd.T.reshape(-1)
            v_abs[sl] += hda.T.reshape(-1)
            v_ne[sl] += 1
            sl = slice(int(cs[v]), int(cs[v + 1]))
            eta[sl] += y
            e_abs[sl] += ya
            e_ne[sl] += 1
    v_extra, e_extra = np.zeros(lam.values.shape[0]), np.zeros(int(cs[-1]))
    touched_v, touched_e = v_ne > 0, e_ne > 0
    if unary and es.unary_factor is not None:
        v = int(es.unary_vertex)
        d = int(cs[v + 1] - cs[v])
        F = np.asarray(es.unary_factor, dtype=dtype).reshape(d, d)      # F[c, k] is U(k, c)
        k = blk[(v, v)]
        sl = slice(int(off[k]), int(off[k + 1]))
        values[sl] += (F @ F.T).T.reshape(-1)
        v_abs[sl] += (np.abs(F) @ np.abs(F).T).T.reshape(-1)
        v_extra[sl] = d
        touched_v[sl] = True
        sl = slice(int(cs[v]), int(cs[v + 1]))
        if es.unary_error is not None:
            eta[sl] += np.asarray(es.unary_error, dtype=dtype)
            e_abs[sl] += np.abs(np.asarray(es.unary_error, dtype=dtype))
        e_extra[sl] = d
        touched_e[sl] = True
    bound_v = (v_ne + 2 * rd + 4 + v_extra) * U53 * v_abs.astype(np.float64)
    bound_e = (e_ne + 2 * rd + 4 + e_extra) * U53 * e_abs.astype(np.float64)
    return values, eta, v_abs, e_abs, bound_v, bound_e, touched_v, touched_e


def fp64_restatement(lam, es, weights=True, unary=True):
    r = reference(lam, es, weights, unary, dtype=np.float64)
    return r[0], r[1]


# ---------------------------------------------------------------------------------------------------------------------
# the cases: every edge list is written down, nothing is drawn
# ---------------------------------------------------------------------------------------------------------------------

def _arr(x):
    return np.asarray(x, dtype=np.int64)


def chain_edges(n, first=0):
    """Odometry first -> first + 1 -> ..., loop closures 3 .. 13 vertices back in alternating orientation, and every 25th
    odometry edge a second and a third time, once in each orientation."""
    v0, v1 = [], []
    for i in range(n - 1):
        v0.append(first + i)
        v1.append(first + i + 1)
        if i % 25 == 7:
            v0 += [first + i + 1, first + i]
            v1 += [first + i, first + i + 1]
    for k, i in enumerate(range(20, n, 7)):
        j = i - (3 + i % 11)
        a, b = (i, j) if k % 2 else (j, i)
        v0.append(first + a)
        v1.append(first + b)
    return v0, v1


CHAIN = frozenset({"multi_edge_block", "flipped_edge"})
LONG_PAIRS = ((2, 6), (2, 7), (2, 3), (3, 3), (6, 6), (7, 7))      # long_kernel_exists()
HUB_EDGES = (95, 96, 97, 256, 257, 513)


def _chain_case(rd, d, groups, name=None, n=200):
    v0, v1 = chain_edges(n)
    has_groups = groups != 0 and (rd, d) not in ((7, 7), (4, 6), (8, 7), (8, 3))
    reached = set(CHAIN)
    if has_groups:
        # (rd 2, d 3: 92 edges fit, the package fills first)
        reached |= {"group_closed_at_vertex_count"} if groups else {"group_closed_at_package_words" if (rd, d) == (2, 3) else "group_closed_at_edge_cap"}
        reached.add("group_kernel_%d" % (rd if rd in (2, 3, 6, 7) else 0))
    else:
        reached |= {"groups_off" if groups == 0 else "no_groups_cap_under_8", "single_entry_record"}
        packed = rd in (2, 3) and 2 * (d * d + d) <= 64
        reached |= {"small_packed" if packed else "plain_diag"}
        reached |= {"offdiag_packed" if rd in (2, 3) and 2 * d * d <= 64 else "offdiag_plain"}
    route = "group" if has_groups else ("small" if rd in (2, 3) and 2 * (d * d + d) <= 64 else "plain")
    return Case(name or "chain-%d-%d-%d" % (rd, d, d), np.full(n, d), _arr(v0), _arr(v1), rd, groups, 5, frozenset(reached),
                frozenset({"long"}), anchor_route=route, seed=rd * 10 + d)


def _ba_edges(n_cams, n_pts, cams_first):
    """Landmark j is seen by 1 + j % 4 cameras."""
    cam, pt = [], []
    for j in range(n_pts):
        for k in range(1 + j % 4):
            cam.append((j * 3 + k * 5) % n_cams)
            pt.append(j)
    cam, pt = _arr(cam), _arr(pt)
    return (cam, pt + n_cams) if cams_first else (cam + n_pts, pt)


def _ba_case(rd, dc, dp, cam_is_v0, groups):
    n_cams, n_pts = 12, 61
    cam, pt = _ba_edges(n_cams, n_pts, True)
    dims = np.concatenate([np.full(n_cams, dc), np.full(n_pts, dp)])
    v0, v1 = (cam, pt) if cam_is_v0 else (pt, cam)
    name = "ba-%d-%d-%d-%s-%s" % (rd, dc, dp, "cam0" if cam_is_v0 else "pt0", "groups" if groups is None else "nogroups")
    if groups is None:
        reached = {"group_kernel_%d" % rd}
        # (rd 3: 12 edges fit, most cameras have more and stay out of the groups)
        anchor, route = (3, "plain" if rd == 3 else "group") if cam_is_v0 else (n_cams + 7, "group")
    else:
        reached = {"groups_off", "small_packed", "offdiag_packed", "single_entry_record"}
        reached.add("plain_diag" if 2 * (dc * dc + dc) > 64 else "small_packed")
        anchor, route = (3, "plain" if 2 * (dc * dc + dc) > 64 else "small") if cam_is_v0 else (n_cams + 7, "small")
    if not cam_is_v0:
        reached.add("flipped_edge")
    return Case(name, dims, v0, v1, rd, groups, anchor, frozenset(reached), frozenset({"long"}), anchor_route=route,
                seed=rd * 100 + dc * 10 + dp + (0 if cam_is_v0 else 1000))


def _star_case(rd, d):
    """Hubs of 95, 96, 97, 256, 257 and 513 edges among vertices of one edge each; the hub is vertex 0 of every other edge;
    the anchor is the hub of 257."""
    v0, v1, hubs, n = [], [], [], 0
    for ne in HUB_EDGES:
        half = ne // 2
        hub = n + half                       # spokes on both sides of the hub's index: both orientations of the stored block
        spokes = [n + i for i in range(ne + 1) if n + i != hub]
        for k, s in enumerate(spokes):
            a, b = (hub, s) if k % 2 == 0 else (s, hub)
            v0.append(a)
            v1.append(b)
        hubs.append(hub)
        n += ne + 1
    reached = {"long", "vertex_over_cap_closes_group", "single_entry_record", "flipped_edge"}
    if (rd, d) != (7, 7):
        reached.add("group_kernel_%d" % rd)
    else:
        reached.add("no_groups_cap_under_8")
    reached.add("small_packed" if rd in (2, 3) and d == 3 else "plain_diag")     # the hub of 95
    if (rd, d) == (7, 7):
        reached.discard("vertex_over_cap_closes_group")
    return Case("star-%d-%d" % (rd, d), np.full(n, d), _arr(v0), _arr(v1), rd, None, hubs[4], frozenset(reached),
                anchor_route="long", seed=rd * 10 + d + 500), hubs


def _two_hub_case(cams_first):
    """A (2, 6, 3) set whose camera 0 sees 100 landmarks and whose landmark 0 is seen by 100 cameras: the dimension of the
    hub with the lower index goes to the long kernel, the other hub to the packed / the one-wave kernel."""
    n_c = n_p = 100
    cam = [0] * n_p + list(range(1, n_c))
    pt = list(range(n_p)) + [0] * (n_c - 1)
    cam, pt = _arr(cam), _arr(pt)
    if cams_first:
        dims = np.concatenate([np.full(n_c, 6), np.full(n_p, 3)])
        v0, v1, anchor = cam, pt + n_c, n_c          # the anchor: the landmark hub (packed)
        reached, route = {"long", "long_dim_taken", "small_packed"}, "small"
    else:
        dims = np.concatenate([np.full(n_p, 3), np.full(n_c, 6)])
        v0, v1, anchor = cam + n_p, pt, n_p          # the anchor: the camera hub (one wave)
        reached, route = {"long", "long_dim_taken", "plain_diag", "flipped_edge"}, "plain"
    return Case("two-hubs-%s" % ("cams-first" if cams_first else "points-first"), dims, v0, v1, 2, None, anchor,
                frozenset(reached | {"vertex_over_cap_closes_group", "group_kernel_2"}),
                anchor_route=route, seed=900 + cams_first)


def _over_cap_case():
    """An SE(3) chain (cap: 16 edges) whose vertex 50 has 20 edges more: it stays out of the groups, between grouped
    neighbours, and is the anchor."""
    n = 120
    v0, v1 = chain_edges(n)
    for k, j in enumerate(range(70, 110, 2)):
        a, b = (50, j) if k % 2 else (j, 50)
        v0.append(a)
        v1.append(b)
    return Case("over-cap-between-groups", np.full(n, 6), _arr(v0), _arr(v1), 6, None, 50,
                frozenset({"vertex_over_cap_closes_group", "group_closed_at_edge_cap", "plain_diag", "offdiag_plain",
                           "group_kernel_6"}), frozenset({"long"}), anchor_route="plain", seed=61)


def _package_words_case():
    """A chain of 2-d residuals between 3-d vertices (cap: 92 edges, so a group would take dozens of vertices) in which the columns of vertices 100 and
    130 hold 60 and 99 blocks no edge touches: the first closes the open group on GRP_PACKAGE_WORDS and starts the next one,
    the second does not fit a package even alone and stays out."""
    n = 160
    v0, v1 = chain_edges(n)
    extra = [(r, 100) for r in range(0, 60)] + [(r, 130) for r in range(0, 99)]
    return Case("package-words", np.full(n, 3), _arr(v0), _arr(v1), 2, None, 100,
                frozenset({"group_closed_at_package_words", "vertex_over_package_closes_group", "edgeless_block",
                           "group_kernel_2", "small_packed", "offdiag_packed"}), frozenset({"long"}), extra_pairs=tuple(extra),
                anchor_route="group", seed=62)


def _beyond_case(groups, name, reached):
    """Lambda larger than the set: a (6, 6, 6) chain on vertices 10 .. 69; vertices 0 .. 9 and 70 .. 79 have no edge, some of
    dimensions 1, 4 and 7; off-diagonal blocks among them and into the chain that no edge touches."""
    n = 80
    dims = np.full(n, 6)
    dims[[0, 3, 72]] = 1
    dims[[1, 4, 75]] = 4
    dims[[2, 5, 78]] = 7
    v0, v1 = chain_edges(60, first=10)
    extra = [(0, 2), (1, 2), (0, 5), (3, 20), (4, 40), (5, 41), (20, 60), (30, 72), (72, 75), (75, 78), (70, 79), (10, 12)]
    return Case(name, dims, _arr(v0), _arr(v1), 6, groups, 30, frozenset(reached), frozenset({"long"}), extra_pairs=tuple(extra),
                anchor_route="group" if groups != 0 else "plain", seed=63)


def _one_edge_case(flip):
    """n_edges = 1: a (2, 6, 3) edge between vertices 2 and 3 (flipped: from vertex 2 back to vertex 0) among vertices without
    an edge, and a block (1, 4) no edge touches."""
    dims, v0, v1 = (np.array([3, 6, 6, 3, 3]), [2], [0]) if flip else (np.array([6, 3, 6, 3, 3]), [2], [3])
    return Case("one-edge-%s" % ("flipped" if flip else "straight"), dims, _arr(v0), _arr(v1), 2, None, 2,
                frozenset({"edgeless_vertex", "edgeless_block", "group_kernel_2"} | ({"flipped_edge"} if flip else set())),
                frozenset({"long"}), extra_pairs=((1, 4),), anchor_route="group", seed=64 + flip)


def _packed_case(rd, da, db, n_a, n_b):
    """Vertices of dimensions da (first n_a) and db, every b seen by 1 .. 3 a's, the groups off: everything goes packed; the
    counts leave the last wave ragged."""
    va, vb = [], []
    for j in range(n_b):
        for k in range(1 + j % 3):
            va.append((j * 2 + k * 3) % n_a)
            vb.append(n_a + j)
    # both orientations need one dimension per side: a's are vertex 0
    dims = np.concatenate([np.full(n_a, da), np.full(n_b, db)])
    return Case("packed-%d-%d-%d" % (rd, da, db), dims, _arr(va), _arr(vb), rd, 0, n_a + 1,
                frozenset({"groups_off", "small_packed", "offdiag_packed", "single_entry_record"}),
                frozenset({"long", "plain_diag", "offdiag_plain"}), anchor_route="small", seed=700 + rd * 100 + da * 10 + db)


def build_cases():
    cases = []
    for rd, d in ((6, 6), (3, 3), (2, 3), (6, 7), (1, 7), (4, 2), (5, 1), (7, 7), (4, 6), (8, 7), (8, 3)):
        cases.append(_chain_case(rd, d, None))
    for g in (0, 1, 2, 3):
        cases.append(_chain_case(6, 6, g, "chain-6-6-6-groups-%d" % g))
    cases.append(_chain_case(3, 3, 0, "chain-3-3-3-groups-0"))
    cases.append(_chain_case(2, 3, 0, "chain-2-3-3-groups-0"))
    for rd, dc, dp in ((2, 6, 3), (2, 7, 3), (2, 3, 2), (3, 6, 3)):
        for cam_is_v0 in (True, False):
            for groups in (None, 0):
                cases.append(_ba_case(rd, dc, dp, cam_is_v0, groups))
    for rd, d in LONG_PAIRS:
        cases.append(_star_case(rd, d)[0])
    cases += [_two_hub_case(True), _two_hub_case(False), _over_cap_case(), _package_words_case()]
    cases.append(_beyond_case(None, "beyond-the-set", {"edgeless_block", "edgeless_vertex", "group_kernel_6"}))
    cases.append(_beyond_case(1, "beyond-the-set-groups-1", {"edgeless_block", "edgeless_vertex", "empty_group_package",
                                                            "group_closed_at_vertex_count", "group_kernel_6"}))
    cases.append(_beyond_case(0, "beyond-the-set-groups-0", {"edgeless_block", "edgeless_vertex", "groups_off", "plain_diag",
                                                            "offdiag_plain"}))
    cases += [_one_edge_case(False), _one_edge_case(True)]
    for rd, da, db, n_a, n_b in ((2, 1, 1, 7, 23), (2, 2, 2, 5, 17), (3, 4, 4, 7, 16), (3, 5, 5, 6, 15), (2, 4, 1, 7, 22),
                                 (3, 5, 2, 5, 19), (2, 2, 5, 9, 14), (3, 1, 4, 8, 21)):
        cases.append(_packed_case(rd, da, db, n_a, n_b))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
