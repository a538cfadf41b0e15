"""CPU replay of the dense top's tile schedule (csrc/tile_schedule.cpp; the kernels that run it: csrc/dense_tiles.hip).

Nothing here comes from the library: the filled pattern and the heights are recomputed, then the tables are replayed launch
by launch in the order tile_cholesky() and tile_backsolve() launch them -- per level the diagonal launch (the level's potrf
tiles and the riders rider_ptr[l] .. rider_ptr[l + 1]), the trsm launch, the urgent update launch; then the backward launches
top down.  replay_symbolic() keeps per tile the source columns applied so far and raises ReplayError at the first broken
rule (the rules are listed in DESIGN.md); replay_numeric() lets the same tables drive numpy tile operations on a random
matrix of the pattern and returns the errors of L and x against numpy's dense factorization.  The designed patterns of the
host test and of tests/test_dense_tiles_gpu.py are built here as well."""
import numpy as np

NB = 64
KNOBS = [(4, 1024), (1, 1), (1, 1024), (64, 1)]  # (rider chunk, rider budget); the first is the default


class ReplayError(AssertionError):
    pass


def _need(cond, *what):
    if not cond:
        raise ReplayError(" ".join(str(w) for w in what))


# ---- patterns ----

def empty(T):
    return np.zeros((T, T), dtype=bool)


def forced(nz):
    """diagonal and last tile row set, lower triangle only"""
    T = nz.shape[0]
    out = np.tril(nz).astype(bool)
    out[np.arange(T), np.arange(T)] = True
    out[T - 1, :] = True
    return out


def chain(T):
    nz = empty(T)
    for i in range(1, T):
        nz[i, i - 1] = True
    return nz


def meet(m):
    """m chains of two columns that meet in the diagonal tile of column 2 m: an urgent target with m sources"""
    nz = empty(2 * m + 2)
    for c in range(m):
        nz[2 * c + 1, 2 * c] = True
        nz[2 * m, 2 * c + 1] = True
    return nz


def binary_tree():
    """complete binary tree of 15 tile columns in nested-dissection order, every column linked to all its ancestors"""
    nz = empty(15)
    def rec(lo, hi, ancestors):  # columns lo .. hi - 1, the root of the subtree last
        root = hi - 1
        for a in ancestors:
            nz[a, root] = True
        if hi - lo > 1:
            half = (hi - 1 - lo) // 2
            rec(lo, lo + half, ancestors + [root])
            rec(lo + half, root, ancestors + [root])
    rec(0, 15, [])
    return nz


def with_fill():
    nz = empty(6)
    nz[2, 0] = nz[4, 0] = True  # fills (4, 2)
    nz[3, 1] = nz[4, 1] = True  # fills (4, 3)
    return nz


def comb():
    """12 leaf columns that all update tile (23, 22); column 22 sits on top of a chain of ten: it is factored ten levels later"""
    nz = empty(25)
    for leaf in range(12):
        nz[22, leaf] = nz[23, leaf] = True
    for i in range(13, 23):
        nz[i, i - 1] = True
    return nz


def designed_patterns():
    return {"one": empty(1), "two": empty(2), "chain8": chain(8), "arrow9": empty(9), "meet2": meet(2), "meet3": meet(3),
            "meet5": meet(5), "tree15": binary_tree(), "full6": np.tril(np.ones((6, 6), dtype=bool)), "fill6": with_fill(),
            "comb25": comb()}


def random_pattern(rng):
    T = int(rng.integers(1, 41))
    density = float(rng.choice([0.0, 0.03, 0.08, 0.15, 0.3, 0.6, 1.0]))
    return np.tril(rng.random((T, T)) < density)


def pattern_text(nz, chunk, budget):
    T = nz.shape[0]
    return "pattern %d %d %d %s\n" % (T, chunk, budget, " ".join(str(int(v)) for v in np.asarray(nz).flatten(order="F")))


def parse_driver_output(text):
    """the cases of one run of tests/tile_schedule_driver.cpp"""
    cases, cur = [], None
    for line in text.splitlines():
        f = line.split()
        if not f:
            continue
        if f[0] == "case":
            cur = {"T": int(f[1]), "chunk": int(f[2]), "budget": int(f[3]), "ok": int(f[4]) != 0, "n_levels": int(f[5])}
        elif f[0] == "end":
            cases.append(cur)
            cur = None
        else:
            v = np.array([int(x) for x in f[2:]], dtype=np.int32)
            assert len(v) == int(f[1]), line[:80]
            if f[0] in ("trsm", "tgt", "riders", "back_diag", "back_carry"):
                v = v.reshape(-1, 4)
            elif f[0] == "nz":
                v = v.reshape(cur["T"], cur["T"]).T.astype(bool)  # column-major flags -> [row, column]
            cur[f[0]] = v
    assert cur is None, "truncated driver output"
    return cases


# ---- the structure, recomputed ----

def fill(nz):
    """filled lower pattern (right-looking symbolic elimination of tiles) and the height of every tile column"""
    T = nz.shape[0]
    F = forced(nz)
    for j in range(T):
        rows = np.nonzero(F[j + 1:, j])[0] + j + 1
        for a in rows:
            F[rows[rows >= a], a] = True
    height = np.zeros(T, dtype=int)
    for i in range(T):
        below = np.nonzero(F[i, :i])[0]
        height[i] = 1 + height[below].max() if len(below) else 0
    return F, height


# ---- symbolic replay ----

def replay_symbolic(nz, t, chunk, budget):
    """replays the tables t (parse_driver_output, or the device tables of the GPU probe) of pattern nz; returns the set of
    schedule forms the tables contain (the keys of REACH)"""
    T = nz.shape[0]
    F, height = fill(nz)
    n_levels = int(height.max()) + 1
    reach = set()
    _need(t["ok"], "the host function reported a contradiction")
    _need(t["n_levels"] == n_levels and np.array_equal(t["height"], height), "heights", t["height"], height)
    for key, n in (("level_potrf_ptr", n_levels + 1), ("level_trsm_ptr", n_levels + 1), ("level_tgt_ptr", n_levels + 1),
                   ("level_urgent_end", n_levels), ("rider_ptr", n_levels + 1), ("back_diag_ptr", n_levels + 1),
                   ("back_carry_ptr", n_levels + 1)):
        p = t[key]
        _need(len(p) == n and (key == "level_urgent_end" or p[0] == 0) and np.all(np.diff(p) >= 0), key, p)
    _need(t["level_potrf_ptr"][-1] == len(t["potrf"]) and t["level_trsm_ptr"][-1] == len(t["trsm"]) and
          t["level_tgt_ptr"][-1] == len(t["tgt"]) and t["rider_ptr"][-1] == len(t["riders"]) and
          t["back_diag_ptr"][-1] == len(t["back_diag"]) and t["back_carry_ptr"][-1] == len(t["back_carry"]), "table lengths")
    src = t["src"]
    applied = {}   # tile -> source columns in the order applied
    done = {}      # tile -> number of the launch that factored (diagonal) or solved (sub-diagonal) it
    jobs_of = {}   # target -> launches in which a rider job worked on it
    n_launch = 0

    def deadline(i1, i2):  # the last diagonal launch whose riders may still write the tile
        return height[i2] - 1 if i1 == i2 else height[i2]

    want = {(int(i1), int(i2)): [int(k) for k in np.nonzero(F[i1, :i2] & F[i2, :i2])[0]] for i1, i2 in zip(*np.nonzero(F))}

    def wanted(i1, i2):  # the source columns of a tile
        return want[(i1, i2)]

    def check_hazards(groups, where):
        """groups: (tiles read, tiles written) per workgroup of one launch"""
        writer = {}
        for g, (_, writes) in enumerate(groups):
            for w in writes:
                _need(w not in writer, where, "tile", w, "is written by two workgroups")
                writer[w] = g
        for g, (reads, _) in enumerate(groups):
            for r in reads:
                _need(writer.get(r, g) == g, where, "tile", r, "is written by one workgroup and read by another")

    def update_job(rec, where):
        i1, i2, s0, s1 = (int(v) for v in rec)
        _need(0 <= i2 <= i1 < T and F[i1, i2], where, "target", (i1, i2), "is outside the pattern")
        _need(0 <= s0 < s1 <= len(src), where, "target", (i1, i2), "has an empty or broken source list", (s0, s1))
        _need((i1, i2) not in done, where, "target", (i1, i2), "is already factored or solved")
        reads = set()
        got = applied.setdefault((i1, i2), [])
        for k in (int(v) for v in src[s0:s1]):
            _need(0 <= k < i2 and F[i1, k] and F[i2, k], where, "source", k, "of", (i1, i2), "is no source of it")
            for tile in ((i1, k), (i2, k)):
                _need(done.get(tile, n_launch) < n_launch, where, "source tile", tile, "of", (i1, i2), "is not complete yet")
                reads.add(tile)
            _need(k not in got, where, "source", k, "is applied to", (i1, i2), "twice")
            got.append(k)
        return (i1, i2), s1 - s0, (reads, {(i1, i2)})

    for l in range(n_levels):
        # the diagonal launch
        where = "level %d, diagonal launch:" % l
        groups = []
        p0, p1 = t["level_potrf_ptr"][l], t["level_potrf_ptr"][l + 1]
        _need(sorted(int(j) for j in t["potrf"][p0:p1]) == [j for j in range(T) if height[j] == l], where, "potrf columns",
              t["potrf"][p0:p1])
        if p1 - p0 >= 3:
            reach.add("level_with_3_potrf")
        for j in (int(v) for v in t["potrf"][p0:p1]):
            _need(sorted(applied.get((j, j), [])) == wanted(j, j), where, "diagonal tile", j, "has received",
                  applied.get((j, j), []), "wants", wanted(j, j))
            groups.append(({(j, j)}, {(j, j)}))
        n_budget = budget
        b_past_due = False
        r0, r1 = t["rider_ptr"][l], t["rider_ptr"][l + 1]
        _need(l > 0 or r1 == r0, "riders in the first launch")
        for rec in t["riders"][r0:r1]:
            target, n_src, group = update_job(rec, where)
            b_due = deadline(*target) <= l
            _need(deadline(*target) >= l, where, "rider", target, "rides behind its deadline")
            if b_due:
                _need(not b_past_due, where, "a due job stands behind one that is not due")
                if n_src > chunk:
                    reach.add("due_job_above_chunk")
            else:
                b_past_due = True
                _need(n_src <= chunk, where, "rider", target, "is not due and takes", n_src, "sources, chunk", chunk)
                _need(n_budget > 0, where, "rider", target, "is not due and the budget is", n_budget)
            n_budget -= n_src
            _need(l not in jobs_of.setdefault(target, []), where, "two jobs for", target)
            jobs_of[target].append(l)
            groups.append(group)
        check_hazards(groups, where)
        for j in (int(v) for v in t["potrf"][p0:p1]):
            _need((j, j) not in done, where, "column", j, "is factored twice")
            done[(j, j)] = n_launch
        # what is due has taken everything available; with budget left at the end (it only falls), nothing that had
        # sources available was passed over
        b_passed_over = False
        for (i1, i2), sources in want.items():
            if (i1, i2) in done or l == 0:  # (this level's own diagonal tiles were served by the level before)
                continue
            got = applied.get((i1, i2), [])
            avail = [k for k in sources if height[k] < l and k not in got]
            if deadline(i1, i2) <= l:
                _need(not avail, where, "due target", (i1, i2), "has not received", avail)
            elif avail and l not in jobs_of.get((i1, i2), []):
                b_passed_over = True
        _need(n_budget <= 0 or not b_passed_over, where, "budget", n_budget, "left and a target with sources was passed over")
        if n_budget <= 0 and b_passed_over:
            reach.add("budget_ran_out")
        if n_budget > 0 and r1 > r0:
            reach.add("budget_left")
        n_launch += 1
        # the trsm launch
        where = "level %d, trsm launch:" % l
        groups = []
        solved_here = []
        for i, j, z, _ in (tuple(int(v) for v in rec) for rec in t["trsm"][t["level_trsm_ptr"][l]:t["level_trsm_ptr"][l + 1]]):
            _need(0 <= j < i < T and F[i, j] and height[j] == l, where, "tile", (i, j), "does not belong to this level")
            _need((i, j) not in done, where, "tile", (i, j), "is solved twice")
            _need(done.get((j, j), n_launch) < n_launch, where, "tile", (i, j), "is solved before its column is factored")
            _need(sorted(applied.get((i, j), [])) == wanted(i, j), where, "tile", (i, j), "has received", applied.get((i, j), []),
                  "wants", wanted(i, j))
            reads, writes = {(i, j), (j, j)}, {(i, j)}
            level_sources = [k for k in range(i) if F[i, k] and height[k] == l]
            if z:
                _need(z == 1 and height[i] == l + 1 and level_sources == [j], where, "z = 1 on", (i, j),
                      "whose row's diagonal tile has the sources", level_sources, "in this level")
                _need((i, i) not in done and j not in applied.get((i, i), []), where, "z = 1 on", (i, j), "applied twice")
                applied.setdefault((i, i), []).append(j)
                reads.add((i, i))
                writes.add((i, i))
                reach.add("trsm_z1")
            elif height[i] == l + 1 and len(level_sources) > 1:
                reach.add("trsm_z0_beside_urgent")
            groups.append((reads, writes))
            solved_here.append((i, j))
        check_hazards(groups, where)
        for tile in solved_here:
            done[tile] = n_launch
        n_launch += 1
        # the urgent update launch
        where = "level %d, update launch:" % l
        groups = []
        g0, gu = t["level_tgt_ptr"][l], t["level_urgent_end"][l]
        _need(g0 <= gu and t["level_tgt_ptr"][l + 1] == gu, where, "targets that no launch reads:", g0, gu, t["level_tgt_ptr"][l + 1])
        for rec in t["tgt"][g0:gu]:
            target, n_src, group = update_job(rec, where)
            _need(target[0] == target[1] and height[target[0]] == l + 1, where, "target", target, "is no diagonal tile of the next level")
            _need(all(height[int(k)] == l for k in src[rec[2]:rec[3]]), where, "target", target, "takes sources of other levels")
            if n_src >= 3:
                reach.add("urgent_with_3_sources")
            groups.append(group)
        check_hazards(groups, where)
        n_launch += 1
    # every tile of the filled pattern exactly once: what tile_zero clears
    tiles = [(int(j), int(j)) for j in t["potrf"]] + [(int(r[0]), int(r[1])) for r in t["trsm"]]
    _need(len(set(tiles)) == len(tiles) and set(tiles) == {(int(i), int(j)) for i, j in zip(*np.nonzero(F))},
          "potrf and trsm are not the filled pattern")
    _need(set(done) == set(tiles), "tiles not factored or solved")
    for tile, got in applied.items():
        _need([height[k] for k in got] == sorted(height[k] for k in got), "sources of", tile, "are not in ascending level:", got)
    if any(len(v) >= 3 for v in jobs_of.values()):
        reach.add("target_over_3_rider_launches")

    # backward substitution, top down
    solved = {}      # column -> launch that produced x
    subtracted = {}  # column k -> ancestors j whose L(j,k)^T x_j has been subtracted from z_k
    touched = set()
    for q in range(n_levels):
        where = "backward launch %d:" % q
        h = n_levels - 1 - q
        diag = [tuple(int(v) for v in r) for r in t["back_diag"][t["back_diag_ptr"][q]:t["back_diag_ptr"][q + 1]]]
        carry = [tuple(int(v) for v in r) for r in t["back_carry"][t["back_carry_ptr"][q]:t["back_carry_ptr"][q + 1]]]
        _need(sorted(r[0] for r in diag) == [k for k in range(T) if height[k] == h], where, "diagonal records", diag)
        written = set()
        for b_diag, rec in [(True, r) for r in diag] + [(False, r) for r in carry]:
            k, j = (rec[0], rec[1]) if b_diag else (rec[1], rec[0])
            _need(0 <= k < T and k not in written, where, "two records write z of column", k)
            written.add(k)
            _need(b_diag or j >= 0, where, "carry record without a source")
            if j >= 0:
                _need(k < j < T and F[j, k], where, "pair", (j, k), "is no tile of the factor")
                _need(j not in subtracted.setdefault(k, []), where, "pair", (j, k), "is subtracted twice")
                _need(solved.get(j, q) < q, where, "pair", (j, k), "reads x of column", j, "before it is solved")
                _need(k not in solved and q <= n_levels - 1 - height[k], where, "pair", (j, k), "comes after column", k, "is solved")
                subtracted[k].append(j)
            _need(rec[2] == int(k not in touched), where, "first-touch flag", rec[2], "on column", k,
                  "which has" + ("" if k in touched else " not"), "been touched")
            reach.add(("diag" if b_diag else "carry") + ("_first" if rec[2] else "_later"))
            touched.add(k)
        for r in diag:
            k = r[0]
            _need(sorted(subtracted.get(k, [])) == [j for j in range(k + 1, T) if F[j, k]], where, "column", k,
                  "is solved with", subtracted.get(k, []), "subtracted")
            solved[k] = q
    _need(len(solved) == T, "columns not solved")
    return reach


REACH = ["level_with_3_potrf", "trsm_z1", "trsm_z0_beside_urgent", "urgent_with_3_sources", "target_over_3_rider_launches",
         "due_job_above_chunk", "budget_ran_out", "budget_left", "carry_first", "carry_later", "diag_first", "diag_later"]


# ---- numeric replay ----

def random_system(nz, n, seed):
    """(A, b): symmetric n x n with the tile pattern nz (entries within +-0.4, diagonally dominant) and a right-hand side"""
    T = nz.shape[0]
    rng = np.random.default_rng(seed)
    mask = np.kron(np.tril(forced(nz)), np.ones((NB, NB)))[:n, :n] != 0
    A = np.tril(np.where(mask, rng.uniform(-0.4, 0.4, (n, n)), 0.0))
    A = A + A.T
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(axis=1) + 1.0
    assert n <= T * NB - 1
    return A, rng.uniform(-1.0, 1.0, n)


def padded_matrix(A, b, n_pad):
    """the layout the kernels take: lower triangle, identity on the padding diagonal, the right-hand side in the last row"""
    n = A.shape[0]
    M = np.zeros((n_pad, n_pad))
    M[:n, :n] = np.tril(A)
    M[np.arange(n, n_pad), np.arange(n, n_pad)] = 1.0
    M[n_pad - 1, :n] = b
    return M


def replay_numeric(nz, t, seed=0, n=None):
    """runs the tables on a random system with numpy tile operations; returns (error of L, error of x) against numpy's
    dense Cholesky and solve"""
    import scipy.linalg as sla
    T = nz.shape[0]
    n_pad = T * NB
    n = n_pad - 1 if n is None else n
    A, b = random_system(nz, n, seed)
    M = padded_matrix(A, b, n_pad)
    last = n_pad - 1
    tile = lambda i, j: M[i * NB:(i + 1) * NB, j * NB:(j + 1) * NB]  # noqa: E731
    src = t["src"]

    def update(rec):
        i1, i2, s0, s1 = (int(v) for v in rec)
        acc = np.zeros((NB, NB))
        for k in src[s0:s1]:
            acc += tile(i1, k) @ tile(i2, k).T
        tile(i1, i2)[...] -= acc

    for l in range(t["n_levels"]):
        for j in t["potrf"][t["level_potrf_ptr"][l]:t["level_potrf_ptr"][l + 1]]:
            D = tile(j, j)
            m = NB - 1 if j == T - 1 else NB  # the right-hand side row is solved, not factored
            sym = np.tril(D[:m, :m]) + np.tril(D[:m, :m], -1).T
            L = np.linalg.cholesky(sym)
            if m < NB:
                D[m, :m] = sla.solve_triangular(L, D[m, :m], lower=True)
                D[m, m] = 1.0
            D[:m, :m] = L
        for rec in t["riders"][t["rider_ptr"][l]:t["rider_ptr"][l + 1]]:
            update(rec)
        for i, j, z, _ in t["trsm"][t["level_trsm_ptr"][l]:t["level_trsm_ptr"][l + 1]]:
            Ljj = np.tril(tile(j, j))
            tile(i, j)[...] = sla.solve_triangular(Ljj, tile(i, j).T, lower=True).T
            if z:
                tile(i, i)[...] -= tile(i, j) @ tile(i, j).T
        for rec in t["tgt"][t["level_tgt_ptr"][l]:t["level_urgent_end"][l]]:
            update(rec)
    L = np.tril(M[:n, :n])
    y = M[last, :].copy()
    y[n:] = 0.0
    z = np.full(n_pad, np.nan)  # (NaN: a record without the first-touch flag that comes first would show)
    x = np.full(n_pad, np.nan)
    for q in range(t["n_levels"]):
        new_x = {}
        recs = [(True, r) for r in t["back_diag"][t["back_diag_ptr"][q]:t["back_diag_ptr"][q + 1]]] + \
               [(False, r) for r in t["back_carry"][t["back_carry_ptr"][q]:t["back_carry_ptr"][q + 1]]]
        for b_diag, rec in recs:
            k, j = (int(rec[0]), int(rec[1])) if b_diag else (int(rec[1]), int(rec[0]))
            zk = (y if rec[2] else z)[k * NB:(k + 1) * NB].copy()
            if j >= 0:
                zk -= tile(j, k).T @ x[j * NB:(j + 1) * NB]
            if b_diag:
                Lkk = np.tril(tile(k, k)).copy()
                if k == T - 1:
                    Lkk[NB - 1, :NB - 1] = 0.0
                new_x[k] = sla.solve_triangular(Lkk, zk, lower=True, trans="T")
            else:
                z[k * NB:(k + 1) * NB] = zk
        for k, v in new_x.items():  # (a launch reads the x of earlier launches only)
            x[k * NB:(k + 1) * NB] = v
    L_ref = np.linalg.cholesky(A)
    x_ref = np.linalg.solve(A, b)
    return (float(np.abs(L - L_ref).max() / np.abs(L_ref).max()), float(np.abs(x[:n] - x_ref).max() / np.abs(x_ref).max()))
