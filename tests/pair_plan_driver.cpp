// Test infrastructure (tests/test_pair_plan_sanitizers.py): the host planning of covariance blocks at arbitrary pairs
// (csrc/pair_plan.cpp) on a chain with loop closures, a grid, a grid with a forced dense top, a chain of mixed block sizes and
// a graph in several pieces, checked against a brute-force walk of parent[].  Built with AddressSanitizer + UBSan on the CPU.
// Prints one line per graph ("<name>: pairs .. passes .. ok") and exits 0, or says what is wrong and exits 1.
#include "pair_plan.h"
#include "driver_graphs.h"
#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: pair %ld: failed: %s (line %d)\n", name, long(k), #cond, __LINE__); return false; } } while(0)

static bool check(const char *name, const Plan &P, const std::vector<int64_t> &rows, const std::vector<int64_t> &cols)
{
	const int64_t n_pairs = int64_t(rows.size());
	int64_t k = -1;
	std::vector<int32_t> sched(size_t(P.n), -1); // (restated here: the schedule index of a column, -1 in the dense top)
	for(size_t sc = 0; sc < P.task_cols.size(); ++ sc)
		sched[size_t(P.task_cols[sc])] = int32_t(sc);
	for(int32_t j = 0; j < P.n; ++ j)
		REQUIRE((sched[size_t(j)] < 0) == (P.dense_dim > 0 && P.dense_pos[size_t(j)] >= 0));
	PairPlan pp;
	plan_pairs(P, pair_sched_pos(P), n_pairs, rows.data(), cols.data(), 48, pp);
	REQUIRE(int64_t(pp.pairs.size()) == n_pairs);
	// every pair is planned once: the passes take consecutive runs of the list
	int64_t n_next = 0;
	for(size_t p = 0; p < pp.passes.size(); ++ p) {
		const TPairPass &pass = pp.passes[p];
		REQUIRE(pass.pair0 == n_next && pass.pair1 > pass.pair0);
		n_next = pass.pair1;
		REQUIRE(pass.kp >= 1 && pass.kp <= 48 && pass.cols.size() == pass.lanes.size());
		REQUIRE(std::set<int32_t>(pass.cols.begin(), pass.cols.end()).size() == pass.cols.size());
		int32_t n_lane = 0;
		bool b_dense = false;
		for(size_t i = 0; i < pass.cols.size(); ++ i) {
			REQUIRE(pass.lanes[i] == n_lane);
			n_lane += P.dim[size_t(pass.cols[i])];
		}
		REQUIRE(n_lane == pass.kp);
		std::set<int32_t> used;
		for(k = pass.pair0; k < pass.pair1; ++ k) {
			const TPairRec &rec = pp.pairs[size_t(k)];
			const int32_t jr = P.pinv[size_t(rows[size_t(k)])], jc = P.pinv[size_t(cols[size_t(k)])];
			// both columns of the pair are in its pass, at the lanes recorded
			const std::vector<int32_t>::const_iterator p_r = std::find(pass.cols.begin(), pass.cols.end(), jr),
				p_c = std::find(pass.cols.begin(), pass.cols.end(), jc);
			REQUIRE(p_r != pass.cols.end() && p_c != pass.cols.end());
			REQUIRE(rec.lane_r == pass.lanes[size_t(p_r - pass.cols.begin())] && rec.lane_c == pass.lanes[size_t(p_c - pass.cols.begin())]);
			REQUIRE(rec.dr == P.dim[size_t(jr)] && rec.dc == P.dim[size_t(jc)]);
			REQUIRE(rec.lane_r + rec.dr <= pass.kp && rec.lane_c + rec.dc <= pass.kp);
			used.insert(jr);
			used.insert(jc);
			b_dense = b_dense || rec.dense;
		}
		REQUIRE(used.size() == pass.cols.size()); // (no column without a pair)
		REQUIRE(b_dense == pass.b_dense);
		k = -1;
	}
	REQUIRE(n_next == n_pairs);
	// the rows of every pair: the intersection of the two paths, in schedule order
	int64_t n_out = 0;
	for(k = 0; k < n_pairs; ++ k) {
		const TPairRec &rec = pp.pairs[size_t(k)];
		const int32_t jr = P.pinv[size_t(rows[size_t(k)])], jc = P.pinv[size_t(cols[size_t(k)])];
		std::set<int32_t> path_r;
		bool b_top_r = false, b_top_c = false, b_top_shared = false;
		for(int32_t x = jr; x >= 0; x = P.parent[size_t(x)]) {
			path_r.insert(x);
			b_top_r = b_top_r || sched[size_t(x)] < 0;
		}
		std::vector<std::pair<int32_t, int32_t> > shared; // (schedule index, column)
		for(int32_t x = jc; x >= 0; x = P.parent[size_t(x)]) {
			b_top_c = b_top_c || sched[size_t(x)] < 0;
			if(!path_r.count(x))
				continue;
			if(sched[size_t(x)] >= 0)
				shared.push_back(std::make_pair(sched[size_t(x)], x));
			else
				b_top_shared = true;
		}
		std::sort(shared.begin(), shared.end());
		REQUIRE(rec.n_rows == int32_t(shared.size()));
		REQUIRE(rec.row0 >= 0 && rec.row0 + rec.n_rows <= int64_t(pp.rows.size()));
		for(size_t q = 0; q < shared.size(); ++ q) {
			const TPairRow &row = pp.rows[size_t(rec.row0) + q];
			REQUIRE(row.cs == int32_t(P.cs_new[size_t(shared[q].second)]) && row.dim == P.dim[size_t(shared[q].second)]);
		}
		REQUIRE((rec.dense != 0) == (b_top_r && b_top_c)); // the dense top is one dense system: every row of it counts once both are in
		REQUIRE(!b_top_shared || rec.dense);
		REQUIRE(rec.out == n_out);
		n_out += int64_t(rec.dr) * rec.dc;
	}
	k = -1;
	REQUIRE(pp.n_out == n_out);
	printf("%s: pairs %ld passes %zu dense_dim %d ok\n", name, long(n_pairs), pp.passes.size(), P.dense_dim);
	return true;
}

static bool run(const char *name, int n, const CEdgeList &edges, const std::vector<int> &dims,
	const PlanOptions &opt, std::mt19937 &rng)
{
	Plan P;
	if(!plan_of_graph(name, n, edges, dims, opt, P))
		return false;
	// seeded pair lists: random pairs, one column against many, diagonal pairs, repeats, a single pair
	const int sizes[] = {1, 7, 64, 300};
	for(int t = 0; t < 4; ++ t) {
		std::vector<int64_t> rows, cols;
		for(int i = 0; i < sizes[t]; ++ i) {
			const int n_kind = int(rng() % 4);
			const int64_t r = int64_t(rng() % unsigned(n)), c = (n_kind == 0)? r : (n_kind == 1)? int64_t(n - 1) : int64_t(rng() % unsigned(n));
			rows.push_back(r);
			cols.push_back(c);
			if(n_kind == 3 && i + 1 < sizes[t]) { // listed twice, the second time transposed
				rows.push_back(c);
				cols.push_back(r);
				++ i;
			}
		}
		if(!check(name, P, rows, cols))
			return false;
	}
	return true;
}

int main()
{
	std::mt19937 rng(7);
	bool b_ok = true;
	{ // chain with loop closures
		int n = 6000;
		const CEdgeList e = chain_with_closures(n, rng);
		b_ok = run("chain", n, e, std::vector<int>(1, 6), PlanOptions(), rng) && b_ok;
		const int mixed[] = {2, 3, 6, 7, 8, 4, 5};
		PlanOptions opt;
		opt.dense_top_nb = 0;
		b_ok = run("mixed", 900, CEdgeList(e.begin(), e.begin() + 899), std::vector<int>(mixed, mixed + 7), opt, rng) && b_ok;
	}
	{ // grid: the default options, and a forced dense top
		int w = 40, n = w * w;
		const CEdgeList e = grid_graph(w);
		b_ok = run("grid", n, e, std::vector<int>(1, 3), PlanOptions(), rng) && b_ok;
		PlanOptions opt;
		opt.dense_top_nb = 4;
		opt.dense_top_auto = false;
		opt.dense_top_min_dim = 0;
		b_ok = run("grid+dense_top", n, e, std::vector<int>(1, 3), opt, rng) && b_ok;
	}
	{ // several pieces and isolated vertices: pairs whose paths never meet
		const CEdgeList e = pieces_graph(rng);
		b_ok = run("pieces", 1500, e, std::vector<int>(1, 6), PlanOptions(), rng) && b_ok;
	}
	return b_ok? 0 : 1;
}
