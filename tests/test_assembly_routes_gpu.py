"""Every route of the device Lambda / eta assembly (csrc/assembly.hip) at small designed shapes (tests/assembly_cases.py):
the group kernel in its instantiations <2>, <3>, <6> and the generic one, the edge-parallel kernel for every (rd, d) it
exists for with lists of 95 .. 513 edges, the packed and the one-wave kernels for diagonal and off-diagonal blocks, single
entries carried in the record, blocks and vertices without an edge.  A case first asserts the route it is about, through
slampp_hip_assembly_get_info against the counts the CPU driver (tests/assembly_tables_driver.cpp) derives for the same
case and against the case's named expectation; then every entry of Lambda and eta against a long-double reference within
a bound derived per entry (assembly_cases.py's docstring), never relative to the largest entry of the array.  Bit
equality is asserted between two runs of one handle, never across routes (the packed diagonal kernel forms (J^T Sigma^-1) J,
the others J^T (Sigma^-1 J))."""
import numpy as np
import pytest
import torch

import assembly_cases as A
from test_assembly_tables_sanitizers import build_driver, run_cases
from slam_plus_plus_amd.hip_solver import CLambdaAssembly_HIP, CLinearSolver_HIP, Refresh_Lambda_sets_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver_counts(tmp_path_factory):
    """The CPU driver's view of every case, computed once (compiled without the sanitizers where their runtime is missing)."""
    directory = tmp_path_factory.mktemp("assembly_routes")
    exe = build_driver(directory) or build_driver(directory, sanitize=False)
    assert exe is not None, "no g++"
    return run_cases(exe, A.CASES, directory)


def dev(a, shift=0):
    """The array on the device; ``shift``: that many doubles into a larger allocation (the pointer is then 8 bytes off)."""
    if a is None:
        return None
    flat = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    t = torch.zeros(flat.shape[0] + shift, dtype=torch.float64, device="cuda")
    t[shift:] = torch.from_numpy(flat).cuda()
    return t[shift:]


class Handle:
    def __init__(self, case, shift=(0, 0, 0, 0)):
        self.case, self.lam, self.es = case, case.structure(), case.edge_set()
        self.solver = CLinearSolver_HIP()
        if case.groups is not None:
            self.solver.set_option("assembly_groups", case.groups)
        self.asm = CLambdaAssembly_HIP(self.solver, self.lam, self.es.v0, self.es.v1, self.es.rd)
        es = self.es
        self.bufs = [dev(a, s) for a, s in zip((es.J0, es.J1, es.sigma_inv, es.err), shift)] + [dev(es.weight)]

    def assemble(self, weights, unary, onto=None):
        """Lambda's values and eta as numpy arrays; ``onto``: (values, eta) held before, accumulated onto."""
        n_values, n_scalars = self.lam.values.shape[0], self.lam.n_scalars
        if onto is None:
            values = torch.full((n_values,), float("nan"), dtype=torch.float64, device="cuda")
            eta = torch.full((n_scalars,), float("nan"), dtype=torch.float64, device="cuda")
        else:
            values, eta = (torch.from_numpy(np.array(a, dtype=np.float64)).cuda() for a in onto)
        p = [b.data_ptr() for b in self.bufs[:4]] + [self.bufs[4].data_ptr() if weights else 0]
        self.asm.Refresh_Lambda_device(*p, values.data_ptr(), eta.data_ptr(), self.es.unary_vertex,
                                       self.es.unary_factor if unary else None, self.es.unary_error if unary else None,
                                       accumulate=onto is not None)
        assert self.solver.sync()
        return values.cpu().numpy(), eta.cpu().numpy()


def within(got, ref, bound, what):
    err = np.abs((got.astype(A.LD) - ref).astype(np.float64))
    bad = ~(err <= bound)                       # (a NaN left behind is bad as well)
    assert not bad.any(), "%s: %d entries outside the bound, the first at %d: got %r, reference %r, error %.3e, bound %.3e" % (
        what, int(bad.sum()), int(np.argmax(bad)), got[np.argmax(bad)], float(ref[np.argmax(bad)]), err[np.argmax(bad)],
        bound[np.argmax(bad)])


def check_handle(h, tag=""):
    """Steps 2 to 5 of a case on one handle."""
    rng = np.random.default_rng(h.case.seed + 4242)
    for weights, unary in ((True, True), (False, False)):
        ref_v, ref_e, abs_v, abs_e, bound_v, bound_e, touched_v, touched_e = A.reference(h.lam, h.es, weights, unary)
        what = "%s%s weights=%d unary=%d" % (h.case.name, tag, weights, unary)
        values, eta = h.assemble(weights, unary)
        within(values, ref_v, bound_v, what + " values")
        within(eta, ref_e, bound_e, what + " eta")
        assert np.all(values[~touched_v] == 0) and np.all(eta[~touched_e] == 0), what   # blocks and vertices without an edge: zeros
        values2, eta2 = h.assemble(weights, unary)
        assert values.tobytes() == values2.tobytes() and eta.tobytes() == eta2.tobytes(), what + ": two runs differ"
        # onto what the arrays hold: held no larger than S_abs, entry by entry; the bound widened by one rounding of the sum
        held_v = rng.uniform(-1, 1, values.shape[0]) * np.where(abs_v > 0, abs_v.astype(np.float64), 1.0)
        held_e = rng.uniform(-1, 1, eta.shape[0]) * np.where(abs_e > 0, abs_e.astype(np.float64), 1.0)
        values3, eta3 = h.assemble(weights, unary, onto=(held_v, held_e))
        sum_v, sum_e = held_v.astype(A.LD) + ref_v, held_e.astype(A.LD) + ref_e
        within(values3, sum_v, bound_v + A.U53 * np.abs(sum_v.astype(np.float64)), what + " accumulated values")
        within(eta3, sum_e, bound_e + A.U53 * np.abs(sum_e.astype(np.float64)), what + " accumulated eta")
        assert values3[~touched_v].tobytes() == held_v[~touched_v].tobytes(), what + ": a block without an edge was touched"
        assert eta3[~touched_e].tobytes() == held_e[~touched_e].tobytes(), what + ": a vertex without an edge was touched"


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_route(case, driver_counts):
    h = Handle(case)
    info = h.asm.info()
    want, routes, reached = driver_counts[case.name]
    assert info == want, (info, want)
    # the case's named routes, from the handle itself
    assert case.reached <= reached
    for name in case.reached:
        if name.startswith("group_kernel_"):
            assert info["n_groups"] > 0 and name == "group_kernel_%d" % (info["rd"] if info["rd"] in (2, 3, 6, 7) else 0)
        if name in ("groups_off", "no_groups_cap_under_8"):
            assert info["n_groups"] == 0 and (name == "groups_off" or info["n_grp_cap_edges"] < 8)
        if name == "long":
            assert info["n_long"] > 0 and info["n_long_dim"] in (info["d0"], info["d1"])
        if name == "small_packed":
            assert info["n_small"] > 0
        if name == "plain_diag":
            assert info["n_plain_diag"] > 0
        if name == "offdiag_packed":
            assert info["n_offdiag"] > 0 and info["b_offdiag_packed"] == 1
        if name == "offdiag_plain":
            assert info["n_offdiag"] > 0 and info["b_offdiag_packed"] == 0
    for name in case.not_reached:
        if name == "long":
            assert info["n_long"] == 0
        if name == "plain_diag":
            assert info["n_plain_diag"] == 0
        if name == "offdiag_plain":
            assert info["n_offdiag"] == 0 or info["b_offdiag_packed"] == 1
    assert sum(routes.count(c) for c in "LSP") == info["n_long"] + info["n_small"] + info["n_plain_diag"]
    check_handle(h)


def test_two_sets_on_one_lambda():
    """slampp_hip_assemble_sets_device_async: an SE(3) chain over the poses (groups <6>) and 2-d observations of landmarks
    from the poses (groups <2>) on one Lambda; the pose-pose blocks belong to the first set alone, the pose-landmark and the
    landmark blocks to the second, the pose blocks to both.  The arrays start as NaN: the call owns their initial state."""
    n_p, n_l = 40, 50
    dims = np.concatenate([np.full(n_p, 6), np.full(n_l, 3)])
    a0, a1 = A.chain_edges(n_p)
    b0 = [(3 * j + 7 * k) % n_p for j in range(n_l) for k in range(1 + j % 3)]
    b1 = [n_p + j for j in range(n_l) for k in range(1 + j % 3)]
    every0, every1 = np.array(a0 + b0, dtype=np.int64), np.array(a1 + b1, dtype=np.int64)
    pairs = tuple(zip(every0.tolist(), every1.tolist()))
    cases = [A.Case("sets-poses", dims, np.array(a0, dtype=np.int64), np.array(a1, dtype=np.int64), 6, None, 7, frozenset(),
                    extra_pairs=pairs, seed=801),
             A.Case("sets-landmarks", dims, np.array(b0, dtype=np.int64), np.array(b1, dtype=np.int64), 2, None, 7, frozenset(),
                    extra_pairs=pairs, seed=802)]
    lam = cases[0].structure()
    assert np.array_equal(lam.brow_idx, cases[1].structure().brow_idx)
    sets = [c.edge_set() for c in cases]
    solver = CLinearSolver_HIP()
    asms = [CLambdaAssembly_HIP(solver, lam, es.v0, es.v1, es.rd) for es in sets]
    assert all(a.info()["n_groups"] > 0 for a in asms)
    bufs = [[dev(a) for a in (es.J0, es.J1, es.sigma_inv, es.err, es.weight)] for es in sets]
    refs = [A.reference(lam, sets[0], True, True), A.reference(lam, sets[1], True, False)]
    ref_v, ref_e = refs[0][0] + refs[1][0], refs[0][1] + refs[1][1]
    bound_v = refs[0][4] + refs[1][4] + A.U53 * np.abs(ref_v.astype(np.float64))     # each set's bound, and the sum's rounding
    bound_e = refs[0][5] + refs[1][5] + A.U53 * np.abs(ref_e.astype(np.float64))
    only_first, only_second = refs[0][6] & ~refs[1][6], refs[1][6] & ~refs[0][6]
    assert only_first.any() and only_second.any() and (refs[0][6] & refs[1][6]).any()
    results = []
    for _ in range(2):
        values = torch.full((lam.values.shape[0],), float("nan"), dtype=torch.float64, device="cuda")
        eta = torch.full((lam.n_scalars,), float("nan"), dtype=torch.float64, device="cuda")
        Refresh_Lambda_sets_device(asms, [[b.data_ptr() for b in bs] for bs in bufs], values.data_ptr(), eta.data_ptr(),
                                   sets[0].unary_vertex, sets[0].unary_factor, sets[0].unary_error)
        assert solver.sync()
        results.append((values.cpu().numpy(), eta.cpu().numpy()))
    values, eta = results[0]
    within(values, ref_v, bound_v, "sets values")
    within(eta, ref_e, bound_e, "sets eta")
    # what only one set touches is that set's own result, to the bound of that set alone
    within(values[only_first], refs[0][0][only_first], refs[0][4][only_first], "sets: blocks of the first set")
    within(values[only_second], refs[1][0][only_second], refs[1][4][only_second], "sets: blocks of the second set")
    assert values.tobytes() == results[1][0].tobytes() and eta.tobytes() == results[1][1].tobytes()


@pytest.mark.parametrize("name", ["chain-2-3-3", "chain-6-6-6", "ba-2-6-3-cam0-groups"])
def test_shifted_edge_arrays_are_refused_where_the_group_kernel_copies_16_bytes(name):
    """Groups and rd 2 or 6: J0, J1, Sigma^-1 and the errors must start at multiples of 16 bytes (include/slampp_hip.h);
    a pointer 8 bytes off is refused by both entry points before anything is enqueued."""
    case = A.BY_NAME[name]
    for which in range(4):
        shift = tuple(int(i == which) for i in range(4))
        h = Handle(case, shift)
        assert h.asm.info()["n_groups"] > 0 and h.bufs[which].data_ptr() % 16 == 8
        values = torch.full((h.lam.values.shape[0],), 7.0, dtype=torch.float64, device="cuda")
        eta = torch.full((h.lam.n_scalars,), 7.0, dtype=torch.float64, device="cuda")
        p = [b.data_ptr() for b in h.bufs]
        with pytest.raises(ValueError):
            h.asm.Refresh_Lambda_device(*p, values.data_ptr(), eta.data_ptr())
        with pytest.raises(ValueError):
            Refresh_Lambda_sets_device([h.asm], [p], values.data_ptr(), eta.data_ptr())
        assert h.solver.sync()
        assert bool((values == 7.0).all()) and bool((eta == 7.0).all())      # not even the sets call's zeroing ran


@pytest.mark.parametrize("name", ["chain-6-6-6-groups-0", "chain-2-3-3-groups-0", "chain-3-3-3", "star-2-6", "chain-1-7-7"])
def test_shifted_edge_arrays_are_taken_elsewhere(name):
    """The same pointers, 8 bytes off, on handles without groups (rd 6 and 2) and on handles whose groups copy 4 bytes at a
    time (rd 3, the generic kernel), and by the edge-parallel kernel, which looks at every record's address: within the
    bound."""
    case = A.BY_NAME[name]
    if name == "star-2-6":      # (its spokes are grouped: rd 2 takes shifted arrays only without groups)
        case = A.dataclasses.replace(case, groups=0, name="star-2-6-groups-0")
    h = Handle(case, (1, 1, 1, 1))
    assert all(b.data_ptr() % 16 == 8 for b in h.bufs[:4])
    info = h.asm.info()
    assert info["n_groups"] == 0 or info["rd"] not in (2, 6)
    check_handle(h, " shifted")
