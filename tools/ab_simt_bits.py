"""Dev helper: the bits the lane-per-task leaf kernels store, of one build, for comparing two builds (a change to the shared column
arithmetic of csrc/simt_device.inl moves every form of the kernels together, so the tests' form-against-form comparisons of one
build cannot see it).

    python3 tools/ab_simt_bits.py dump OUT.npz      # the build of the tree this file lies in (copy the file into the other tree)
    python3 tools/ab_simt_bits.py compare A.npz B.npz

Dumps the factor from factorize() and the solution x for the cases of tests/test_factor_simt_ahead_gpu.py (chain_short,
chain_tall, hub_tall, islands) with the lane-per-task options and the knobs SLAMPP_HIP_DEV_SIMT_FACTOR_AHEAD, _FACTOR_BRANCHES,
SLAMPP_HIP_DEV_SIMT_BWD_AHEAD at 0 0 0, at 1 0 1 and at 1 1 1, and for chain3 and chain7, where the base kernels run with D = 3, 7
and one lane per task; each once before the handle's first kept-factor solve (the kernels that do not store inv(L_jj)) and once
after it (the ones that do, with a second right-hand side on the kept factor), together with the forms the launches say they
took.  compare asks np.array_equal of every array."""
import os as _os; _os.environ.setdefault("SLAMPP_HIP_DEV", "1")  # development options and knobs are refused without it (csrc/plan.h)
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("SLAMPP_HIP_DEV_SIMT_FACTOR_AHEAD", "SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES", "SLAMPP_HIP_DEV_SIMT_BWD_AHEAD")
SETTINGS = ((0, 0, 0), (1, 0, 1), (1, 1, 1))


def launches_of(run):
    """run()'s result, and the forms the lane-per-task launches say they took on stderr (SLAMPP_HIP_STAGE_TIMING), in their order."""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            result = run()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    forms = [("factor " if kind != "backward" else "backward ") + ("branches" if kind == "factor branches" else form)
             for kind, form in re.findall(r"stage_timing lane-per-task (factor branches|factor|backward) launch: .*?(fetch ahead|fetch by column|members)$", text, re.M)]
    return result, ", ".join(forms)


def dump(path):
    os.environ["SLAMPP_HIP_STAGE_TIMING"] = "1"  # (read at analysis: the launches then say which form they take)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import variant_util as V
    import test_factor_simt_ahead_gpu as T
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    cases = {case: T.CASES[case] for case in ("chain_short", "chain_tall", "hub_tall", "islands")}
    cases.update({name: (name, V.PLAN_OPTIONS) for name in ("chain3", "chain7")})
    out = {}
    for case, (name, options) in cases.items():
        lam = V.SYSTEMS[name]() if name in V.SYSTEMS else T.islands()
        solver = CLinearSolver_HIP(**dict(options, **T.LANES))
        assert solver.SymbolicDecomposition_Blocky(lam)
        # the first kept-factor solve of a handle switches the storing of inv(L_jj) on, the b_linv instantiation of the factor
        # kernels, for every factorization after it: one round of the settings without the inverses, one with
        for stored in ("no inverses", "inverses"):
            for setting in SETTINGS:
                os.environ.update({k: str(v) for k, v in zip(KNOBS, setting)})
                x, again = lam.rhs.copy(), -2.0 * lam.rhs

                def run():
                    assert solver.Solve_PosDef_Blocky(lam, x)
                    assert stored == "no inverses" or solver.Solve_Again(again)  # a second right-hand side on the kept factor
                    ok, _, l_values = solver.factorize(lam)
                    assert ok
                    return np.asarray(l_values)
                l_values, forms = launches_of(run)
                key = f"{case} knobs {' '.join(map(str, setting))} {stored}"
                out[key + " x"], out[key + " L"], out[key + " launches"] = x, l_values, np.array(forms)
                if stored == "inverses":
                    out[key + " x again"] = again
                print(f"{key}: x {x.shape[0]} doubles, L {l_values.shape[0]} doubles; {forms}", flush=True)
            x = lam.rhs.copy()
            assert solver.Solve_Again(x)
    np.savez(path, **out)


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    n_differ = 0
    for key in a.files:
        same = a[key].shape == b[key].shape and np.array_equal(a[key], b[key])
        n_differ += not same
        print(f"{key}: {'equal' if same else 'DIFFERENT'}" + (f" ({a[key]})" if key.endswith("launches") else ""))
    print(f"{len(a.files)} arrays, {n_differ} differ")
    return n_differ == 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
