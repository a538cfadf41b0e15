"""The cases of tests/test_schur_variants_gpu.py: for every job shape of the landmark-major Schur assembly
(csrc/schur_tiles.hip) the smallest BA system that produces it, as camera lists (schur_variant_util.Design).  The host test
tests/test_schur_variant_systems_host.py checks every one of them on the CPU: positive definite, cond_2 <= 1e6, oracle and
refined reference agree.

OB = 64 / DC observations a block of a run job: 10 / 9 / 21 for DC = 6 / 7 / 3."""
from schur_variant_util import Case, Design, NT_BUCKETS, TILE_MAX_K, ob_of, tile_loads

DIAG_LENGTHS = [1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65]   # tails of GROUP 8 and 4 and of a quad, pieces of 32 and of 64
REDUCE_COUNTS = [1, 2, 3, 4, 23, 24, 25, 63, 64, 65, 130]       # partial blocks of one block of S: 24 a pass, 64 indices a load
MULT = "SLAMPP_HIP_DEV_RUN_PIECE_MULT"
NO_QUAD, NO_QUAD_WIDE = "SLAMPP_HIP_DEV_NO_QUAD_RUNS", "SLAMPP_HIP_DEV_NO_QUAD_WIDE"
TILE_POINTS_KNOB = "SLAMPP_HIP_DEV_TILE_POINTS"
# the longest camera list of a tile case, by the NL (64-lane loads a landmark) it makes the tile launch take; (3, 2) blocks
# are six doubles: ten of them fit one load, NL = 2 .. 4 do not exist for them, and NL = 4 exists for (7, 3) only
TILE_KMAX = {6: {1: 3, 2: 7, 3: 10}, 7: {1: 3, 2: 6, 3: 9, 4: 10}, 3: {1: 10}}

CASES = {}


def window(first, k):
    return list(range(first, first + k))


# ---- diagonal run jobs, equal lists (schur_tiles = 3): first and last k of every NT bucket, thirteen run lengths --------------

def _diag(bucket, end):
    def design(dc):
        k = NT_BUCKETS[dc][bucket][end]
        d = Design(dc)
        for i, n in enumerate(DIAG_LENGTHS):           # run i on cameras i .. i + k - 1: equal length, so no list continues another
            d.run(window(i, k), [(k, n)])
        return d.finish(10 * bucket + end)
    return design


for _b in range(4):
    for _e, _end in enumerate(("first", "last")):
        CASES[f"diag_nt{_b + 1}_{_end}_k"] = Case(_diag(_b, _e), mode=3, seed=10 * _b + _e)


# ---- sub-pieces: a job of 128 or 129 landmarks keeps its sums across sub-pieces of 64 -------------------------------------------

def _subpieces(k_of):
    def design(dc):
        k = k_of(dc)
        d = Design(dc)
        for i, n in enumerate((64, 65, 128, 129)):
            d.run(window(3 * i, k), [(k, n)])
        return d.finish(40 + k)
    return design


for _m in (2, 4):
    CASES[f"subpieces_mult{_m}_k3"] = Case(_subpieces(lambda dc: 3), mode=3, knobs={MULT: _m}, mult=_m, seed=40 + _m)
    CASES[f"subpieces_mult{_m}_kOB"] = Case(_subpieces(ob_of), mode=3, knobs={MULT: _m}, mult=_m, seed=45 + _m)


# ---- off-diagonal jobs, equal lists: k = OB + 1, 2 OB, 2 OB + 1, 3 OB; runs of 1 .. 5 landmarks (GROUP 2) ------------------------

def _offdiag(k_of):
    def design(dc):
        k = k_of(ob_of(dc))
        d = Design(dc)
        for i in range(5):                                 # five different lists of k of the system's k + 2 cameras
            d.run([c for c in range(k + 2) if c not in (i, k + 1 - i)], [(k, i + 1)])
        return d.finish(50 + k)
    return design


CASES["offdiag_k_OB+1"] = Case(_offdiag(lambda ob: ob + 1), mode=3, seed=51)
CASES["offdiag_k_2OB"] = Case(_offdiag(lambda ob: 2 * ob), mode=3, seed=52)
CASES["offdiag_k_2OB+1"] = Case(_offdiag(lambda ob: 2 * ob + 1), mode=3, seed=53)
# (different lists of 3 OB = 63 cameras at 3 x 3 blocks take 65 cameras: more than the 45 the other systems stay under)
CASES["offdiag_k_3OB"] = Case(_offdiag(lambda ob: 3 * ob), mode=3, seed=54, cams=(12, 65))


# ---- prefix runs: chains of classes whose lists continue one another ---------------------------------------------------------

def _prefix(dc):
    ob = ob_of(dc)
    d = Design(dc)
    for first, last in NT_BUCKETS[dc]:                     # ends inside the first row block, within one NT class (6 x 6: 9 and 10)
        d.run(window(0, last), [(last, 4), (first, 5)])
    d.run(window(1, ob + 1), [(ob + 1, 3), (ob, 3)])       # ends exactly at a block boundary: OB beside OB + 1
    d.run(window(2, 2 * ob + 1), [(2 * ob + 1, 2), (ob + 3, 2)])   # ends inside the third and inside the second block
    # a quad that mixes three lengths (landmarks 0 .. 3), and one whose four landmarks all end right behind the block
    # boundary, before the last row tile of row block 1 (landmarks 4 .. 7: the n_rt_own skip)
    d.run(window(3, ob + 8), [(ob + 8, 2), (ob + 5, 1), (ob + 2, 1), (ob + 1, 4)])
    d.run(window(4, ob + 4), [(ob + 4, 1), (ob + 2, 1)])   # exactly two long tracks: a run also where the default asks for four
    d.listed(window(5, ob + 3))                            # a lone long track: no run, too long for a tile
    return d.finish(60)


CASES["prefix_mode1"] = Case(_prefix, mode=1, seed=60, run_of_interest=6)
CASES["prefix_auto"] = Case(_prefix, mode=-1, seed=60, run_of_interest=6)


# ---- one landmark per step: every NT, diagonal and off-diagonal, with the quads switched off -----------------------------------

def _noquad(chains):
    def design(dc):
        ob = ob_of(dc)
        d = Design(dc)
        for i, (first, last) in enumerate(NT_BUCKETS[dc]):
            d.run(window(i, last), [(last, 5), (first, 4)] if chains else [(last, 9)])
        d.run(window(4, ob + 2), [(ob + 2, 3), (ob + 1, 2)] if chains else [(ob + 2, 5)])
        return d.finish(70 + chains)
    return design


for _knob, _name in ((NO_QUAD, "noquad_runs"), (NO_QUAD_WIDE, "noquad_wide")):
    CASES[_name] = Case(_noquad(0), mode=3, knobs={_knob: 1}, seed=70)
    CASES[_name + "_prefix"] = Case(_noquad(1), mode=3, knobs={_knob: 1}, seed=71)


# ---- tiles (schur_tiles = 2): neighbouring landmarks with overlapping, unequal lists ------------------------------------------

def _tiles(nl, n_cams=16, n_points=60):
    def design(dc):
        kmax = TILE_KMAX[dc][nl]
        d = Design(dc)
        for i in range(n_points):
            d.tile(window((i // kmax) % (n_cams - kmax + 1), 1 + i % kmax))   # 1 .. kmax cameras from one first camera, then from the next
        d.tile(window(n_cams - kmax, kmax))
        return d.finish(80 + nl)
    return design


def _tiles_line(nl):
    return lambda dc, dp: {"NL": nl, "max_k": TILE_KMAX[dc][nl]}


for _nl in (1, 2, 3, 4):
    CASES[f"tiles_nl{_nl}"] = Case(_tiles(_nl), mode=2, tiles=_tiles_line(_nl), route="tile", seed=80 + _nl)


def _tile_shapes(dc):
    d = Design(dc)
    d.tile([])                                 # a landmark nobody sees: no block of S, dl = C^-1 l
    d.tile(window(0, 10))                      # 55 blocks
    d.tile(window(10, 3))                      # + 6 = 61
    d.tile(window(13, 2))                      # + 3: the tile closes at exactly 64 blocks
    d.tile([15], 65)                           # the first would make it 65 and opens the next; 64 landmarks fill that one, the 65th opens a third
    d.listed(window(0, TILE_MAX_K + 1))        # eleven cameras: no tile takes it
    return d.finish(90)


CASES["tile_shapes"] = Case(_tile_shapes, mode=2, route="tile", seed=90,
                            tiles=lambda dc, dp: {"NL": tile_loads(dc, dp, 10), "tiles": 3, "max_slots": 64, "max_k": 10, "max_points": 64})
CASES["tile_one_point"] = Case(_tiles(1, n_points=40), mode=2, knobs={TILE_POINTS_KNOB: 1}, route="tile", seed=91,
                               tiles=lambda dc, dp: {"tiles": 41, "max_points": 1})


# ---- the reduction: one off-diagonal block of S and two diagonal ones with 1 .. 130 partial blocks each ------------------------
# pair j of cameras (2 j, 2 j + 1) is seen by REDUCE_COUNTS[j] different lists, each with a third camera of its own from a
# pool of 130 (so the systems have 152 cameras); every list is a job or a tile of its own and leaves one partial block

def _reduce(both):
    def design(dc):
        d = Design(dc)
        for j, n in enumerate(REDUCE_COUNTS):
            for i in range(n):
                cams = [2 * j, 2 * j + 1, 2 * len(REDUCE_COUNTS) + i]
                if not both:
                    d.run(cams, [(3, 1)])              # schur_tiles = 3: a single landmark is a run
                elif i % 2 == 0:
                    d.run(cams, [(3, 2)])              # schur_tiles = 1: two equal lists are a run ...
                else:
                    d.tile(cams)                       # ... a single one goes to a tile, here of one landmark
        return d.finish(95 + both)
    return design


def _reduce_lengths(dc):
    return {"off_diagonal": {n: 1 for n in REDUCE_COUNTS}, "diagonal": {n: 2 for n in REDUCE_COUNTS}}


CASES["reduce_runs"] = Case(_reduce(0), mode=3, reduce=_reduce_lengths, cams=(152, 152), seed=95)
CASES["reduce_runs_and_tiles"] = Case(_reduce(1), mode=1, knobs={TILE_POINTS_KNOB: 1}, reduce=_reduce_lengths, cams=(152, 152), seed=96,
                                      tiles=lambda dc, dp: {"NL": 1, "max_points": 1, "max_k": 3})


# ---- the default's own gates (schur_tiles = -1) ---------------------------------------------------------------------------------

def _three_and_four(dc):
    d = Design(dc)
    d.tile([0, 1, 2], 3)                       # three equal lists are no run: a tile (18 contributions in 6 blocks: kept)
    for i in range(1, 4):
        d.run(window(3 * i, 3), [(3, 4)])      # four are
    return d.finish(100)


def _half(n_runs):
    def design(dc):
        d = Design(dc)
        for i in range(n_runs):
            d.run(window(3 * i, 3), [(3, 4)])  # 24 contributions a run
        d.listed(window(1, 11))                # 66 contributions each, on the lists whatever happens
        d.listed(window(2, 11))
        return d.finish(101 + n_runs)
    return design


def _dropped_tile(dc):
    d = Design(dc)
    for t in range(2, 22):
        d.tile([0, 1, t], 3)                   # 60 landmarks, 360 contributions in 63 blocks: kept
    for i in range(6):
        d.listed([22 + 2 * i, 23 + 2 * i])     # the next would make it 66 blocks: a tile of their own, 18 contributions in 18 blocks: dropped
    return d.finish(110)


def _nothing_to_share(n_pairs, more):
    def design(dc):
        d = Design(dc)
        for i in range(n_pairs):
            d.listed([2 * i, 2 * i + 1])       # one tile, 3 contributions in 3 blocks a landmark: dropped
        if more:
            d.listed(window(2 * n_pairs, 3))   # a list of another length: whether a run exists is no longer known beforehand
        return d.finish(111)
    return design


# no run and no tile: decided before the classes are formed where every list is as long as every other, after them otherwise
CASES["auto_runs_impossible"] = Case(_nothing_to_share(6, 0), mode=-1, seed=111, lists_keep="runs_impossible", route="list")
CASES["auto_no_jobs"] = Case(_nothing_to_share(5, 1), mode=-1, seed=112, lists_keep="no_jobs", route="list")
CASES["auto_three_no_run_four_a_run"] =Case(_three_and_four, mode=-1, seed=100, tiles=lambda dc, dp: {"tiles": 1, "max_points": 3, "max_slots": 6})
CASES["auto_just_over_half"] = Case(_half(6), mode=-1, seed=101)             # 144 of 276 contributions in runs
CASES["auto_just_under_half"] = Case(_half(5), mode=-1, seed=102, lists_keep="under_half", route="list")   # 120 of 252
CASES["auto_dropped_tile"] = Case(_dropped_tile, mode=-1, route="tile", seed=110,
                                  tiles=lambda dc, dp: {"tiles": 1, "max_points": 60, "max_slots": 63})


# ---- all routes in one system: runs, prefix runs, tiles and lists add to the same blocks of S ------------------------------------

def _all_routes(mode):
    def design(dc):
        first, last = NT_BUCKETS[dc][1]
        d = Design(dc)
        run = d.run if mode != 2 else (lambda cams, classes: [d.tile(cams[:k], n) for k, n in classes])
        run(window(0, 4), [(4, 8)])
        run(window(4, last), [(last, 4), (first, 4)])
        pool = (12, 13, 14, 15)
        for a in range(4):
            for b in range(a + 1, 4):              # six different lists that share 28 blocks: 90 contributions, a tile the default keeps
                cams = [0, 1, 2, pool[a], pool[b]]
                if mode == 3:
                    d.run(cams, [(5, 1)])
                else:
                    d.tile(cams)
        if mode == 3:
            d.run(window(1, 11), [(11, 1)])        # runs only, of any length
        else:
            d.listed(window(1, 11))
        return d.finish(120)
    return design


for _mode, _name in ((-1, "auto"), (1, "mode1"), (2, "mode2"), (3, "mode3")):
    CASES[f"all_routes_{_name}"] = Case(_all_routes(_mode), mode=_mode, seed=120, route="tile" if _mode == 2 else "run",
                                        run_of_interest=1,
                                        tiles=None if _mode == 3 else (lambda dc, dp, m=_mode: {"max_k": max(5, NT_BUCKETS[dc][1][1]) if m == 2 else 5}))


def case_dims():
    """(case, (cam_dim, pt_dim)) of every test: each case at each block size, but for the NL a block size does not have."""
    from schur_variant_util import DIMS
    out = []
    for name in CASES:
        for dims in DIMS:
            if name.startswith("tiles_nl") and int(name[len("tiles_nl"):]) not in TILE_KMAX[dims[0]]:
                continue
            out.append((name, dims))
    return out
