// Test infrastructure (tests/test_pair_sets_plan_sanitizers.py): the host planning of covariance blocks at pairs of column
// sets (plan_pair_sets, csrc/pair_plan.cpp) -- a column is a set of source block columns and a scalar width, as the camera
// and landmark columns of a BA system are over its reduced camera system -- on a band, a band with a forced dense top, a star
// and a graph of two components, checked against a brute-force union and intersection of the paths in parent[].  Built with
// AddressSanitizer + UBSan on the CPU.  Prints one line per graph and list ("<name>: pairs .. passes .. ok") and exits 0,
// or says what is wrong and exits 1.
#include "pair_plan.h"
#include "driver_graphs.h"
#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: pair %ld: failed: %s (line %d)\n", name, long(k), #cond, __LINE__); return false; } } while(0)

struct TSets {
	std::vector<int64_t> ptr;
	std::vector<int32_t> src, width;
	int32_t n() const { return int32_t(width.size()); }
};

static std::set<int32_t> reach_of(const Plan &P, const TSets &sets, int32_t i)
{
	std::set<int32_t> reach;
	for(int64_t q = sets.ptr[size_t(i)]; q < sets.ptr[size_t(i) + 1]; ++ q) {
		for(int32_t x = sets.src[size_t(q)]; x >= 0; x = P.parent[size_t(x)])
			reach.insert(x);
	}
	return reach;
}

static bool check(const char *name, const Plan &P, const TSets &sets, const std::vector<int32_t> &rows, const std::vector<int32_t> &cols)
{
	const int64_t n_pairs = int64_t(rows.size());
	int64_t k = -1;
	const std::vector<int32_t> sched = pair_sched_pos(P);
	PairPlan pp;
	plan_pair_sets(P, sched, n_pairs, rows.data(), cols.data(), sets.n(), sets.ptr.data(), sets.src.data(), sets.width.data(), 48, pp);
	REQUIRE(int64_t(pp.pairs.size()) == n_pairs);
	int64_t n_next = 0;
	for(size_t p = 0; p < pp.passes.size(); ++ p) {
		const TPairPass &pass = pp.passes[p];
		REQUIRE(pass.pair0 == n_next && pass.pair1 > pass.pair0);
		n_next = pass.pair1;
		REQUIRE(pass.kp >= 1 && pass.kp <= 48 && pass.cols.size() == pass.lanes.size());
		REQUIRE(std::set<int32_t>(pass.cols.begin(), pass.cols.end()).size() == pass.cols.size());
		int32_t n_lane = 0;
		std::set<int32_t> want_srcs;
		for(size_t i = 0; i < pass.cols.size(); ++ i) { // the lanes: the sets' widths one after the other
			REQUIRE(pass.cols[i] >= 0 && pass.cols[i] < sets.n());
			REQUIRE(pass.lanes[i] == n_lane);
			n_lane += sets.width[size_t(pass.cols[i])];
			for(int64_t q = sets.ptr[size_t(pass.cols[i])]; q < sets.ptr[size_t(pass.cols[i]) + 1]; ++ q)
				want_srcs.insert(sets.src[size_t(q)]);
		}
		REQUIRE(n_lane == pass.kp);
		// the sources of the pass: those of its sets, each once
		REQUIRE(std::set<int32_t>(pass.srcs.begin(), pass.srcs.end()) == want_srcs && pass.srcs.size() == want_srcs.size());
		std::set<int32_t> used;
		bool b_dense = false;
		for(k = pass.pair0; k < pass.pair1; ++ k) {
			const TPairRec &rec = pp.pairs[size_t(k)];
			const int32_t sr = rows[size_t(k)], sc = cols[size_t(k)];
			const std::vector<int32_t>::const_iterator p_r = std::find(pass.cols.begin(), pass.cols.end(), sr),
				p_c = std::find(pass.cols.begin(), pass.cols.end(), sc);
			REQUIRE(p_r != pass.cols.end() && p_c != pass.cols.end());
			REQUIRE(rec.lane_r == pass.lanes[size_t(p_r - pass.cols.begin())] && rec.lane_c == pass.lanes[size_t(p_c - pass.cols.begin())]);
			REQUIRE(rec.dr == sets.width[size_t(sr)] && rec.dc == sets.width[size_t(sc)]);
			REQUIRE(rec.lane_r + rec.dr <= pass.kp && rec.lane_c + rec.dc <= pass.kp);
			used.insert(sr);
			used.insert(sc);
			b_dense = b_dense || rec.dense;
		}
		REQUIRE(used.size() == pass.cols.size());
		REQUIRE(b_dense == pass.b_dense);
		if(p + 1 < pp.passes.size()) { // greedy: the first pair of the next pass would not have fitted
			const int32_t sr = rows[size_t(pass.pair1)], sc = cols[size_t(pass.pair1)];
			int n_more = used.count(sr)? 0 : sets.width[size_t(sr)];
			if(sc != sr && !used.count(sc))
				n_more += sets.width[size_t(sc)];
			REQUIRE(pass.kp + n_more > 48);
		}
		k = -1;
	}
	REQUIRE(n_next == n_pairs);
	// the rows of every pair: the intersection of the two reaches, in schedule order
	int64_t n_out = 0;
	for(k = 0; k < n_pairs; ++ k) {
		const TPairRec &rec = pp.pairs[size_t(k)];
		const std::set<int32_t> reach_r = reach_of(P, sets, rows[size_t(k)]), reach_c = reach_of(P, sets, cols[size_t(k)]);
		bool b_top_r = false, b_top_c = false;
		for(std::set<int32_t>::const_iterator p_x = reach_r.begin(); p_x != reach_r.end(); ++ p_x)
			b_top_r = b_top_r || sched[size_t(*p_x)] < 0;
		std::vector<std::pair<int32_t, int32_t> > shared; // (schedule index, column)
		for(std::set<int32_t>::const_iterator p_x = reach_c.begin(); p_x != reach_c.end(); ++ p_x) {
			b_top_c = b_top_c || sched[size_t(*p_x)] < 0;
			if(reach_r.count(*p_x) && sched[size_t(*p_x)] >= 0)
				shared.push_back(std::make_pair(sched[size_t(*p_x)], *p_x));
		}
		std::sort(shared.begin(), shared.end());
		REQUIRE(rec.n_rows == int32_t(shared.size()));
		REQUIRE(rec.row0 >= 0 && rec.row0 + rec.n_rows <= int64_t(pp.rows.size()));
		for(size_t q = 0; q < shared.size(); ++ q) {
			const TPairRow &row = pp.rows[size_t(rec.row0) + q];
			REQUIRE(row.cs == int32_t(P.cs_new[size_t(shared[q].second)]) && row.dim == P.dim[size_t(shared[q].second)]);
		}
		REQUIRE((rec.dense != 0) == (b_top_r && b_top_c));
		REQUIRE(rec.out == n_out);
		n_out += int64_t(rec.dr) * rec.dc;
	}
	k = -1;
	REQUIRE(pp.n_out == n_out);
	printf("%s: pairs %ld passes %zu dense_dim %d ok\n", name, long(n_pairs), pp.passes.size(), P.dense_dim);
	return true;
}

// sets of one source each, as wide as that block column: the records of plan_pairs
static bool check_single_source(const char *name, const Plan &P, std::mt19937 &rng)
{
	int64_t k = -1;
	TSets sets;
	for(int32_t j = 0; j < P.n; ++ j) {
		sets.ptr.push_back(j);
		sets.src.push_back(j);
		sets.width.push_back(P.dim[size_t(j)]);
	}
	sets.ptr.push_back(P.n);
	std::vector<int64_t> rows, cols;
	std::vector<int32_t> set_r, set_c;
	for(int i = 0; i < 200; ++ i) {
		const int64_t r = int64_t(rng() % unsigned(P.n)), c = (i % 5 == 0)? r : int64_t(rng() % unsigned(P.n));
		rows.push_back(r);
		cols.push_back(c);
		set_r.push_back(P.pinv[size_t(r)]);
		set_c.push_back(P.pinv[size_t(c)]);
	}
	const std::vector<int32_t> sched = pair_sched_pos(P);
	PairPlan a, b;
	plan_pairs(P, sched, int64_t(rows.size()), rows.data(), cols.data(), 48, a);
	plan_pair_sets(P, sched, int64_t(rows.size()), set_r.data(), set_c.data(), sets.n(), sets.ptr.data(), sets.src.data(),
		sets.width.data(), 48, b);
	REQUIRE(a.n_out == b.n_out && a.pairs.size() == b.pairs.size() && a.rows.size() == b.rows.size() && a.passes.size() == b.passes.size());
	for(k = 0; k < int64_t(a.pairs.size()); ++ k) {
		const TPairRec &x = a.pairs[size_t(k)], &y = b.pairs[size_t(k)];
		REQUIRE(x.out == y.out && x.row0 == y.row0 && x.n_rows == y.n_rows && x.lane_r == y.lane_r && x.lane_c == y.lane_c &&
			x.dr == y.dr && x.dc == y.dc && x.dense == y.dense);
	}
	for(k = 0; k < int64_t(a.rows.size()); ++ k)
		REQUIRE(a.rows[size_t(k)].cs == b.rows[size_t(k)].cs && a.rows[size_t(k)].dim == b.rows[size_t(k)].dim);
	for(k = 0; k < int64_t(a.passes.size()); ++ k) {
		const TPairPass &x = a.passes[size_t(k)], &y = b.passes[size_t(k)];
		REQUIRE(x.kp == y.kp && x.cols == y.cols && x.lanes == y.lanes && x.pair0 == y.pair0 && x.pair1 == y.pair1 && x.b_dense == y.b_dense);
		REQUIRE(std::set<int32_t>(y.srcs.begin(), y.srcs.end()) == std::set<int32_t>(y.cols.begin(), y.cols.end()));
	}
	printf("%s: single-source sets as plan_pairs: pairs %zu passes %zu ok\n", name, a.pairs.size(), a.passes.size());
	return true;
}

static bool run(const char *name, int n, const CEdgeList &edges, int n_dim, const PlanOptions &opt, std::mt19937 &rng)
{
	Plan P;
	if(!plan_of_graph(name, n, edges, std::vector<int>(1, n_dim), opt, P))
		return false;
	// the columns: every block column alone ("cameras", as wide as it is), then sets of 2 .. 30 sources -- neighbours,
	// scattered ones, one that holds every column -- three or two scalars wide ("landmarks")
	TSets sets;
	sets.ptr.push_back(0);
	for(int32_t j = 0; j < n; ++ j) {
		sets.src.push_back(j);
		sets.ptr.push_back(int64_t(sets.src.size()));
		sets.width.push_back(n_dim);
	}
	const int n_wide = 150;
	for(int i = 0; i < n_wide; ++ i) {
		const int n_src = (i == 0)? n : 2 + int(rng() % 29);
		std::set<int32_t> src;
		const int32_t j0 = int32_t(rng() % unsigned(n));
		for(int q = 0; int(src.size()) < std::min(n_src, n); ++ q)
			src.insert((i == 0)? q : (i % 2)? int32_t((j0 + q) % n) : int32_t(rng() % unsigned(n)));
		sets.src.insert(sets.src.end(), src.begin(), src.end());
		sets.ptr.push_back(int64_t(sets.src.size()));
		sets.width.push_back((n_dim > 3)? 3 : 2);
	}
	const int sizes[] = {1, 9, 80, 400};
	for(int t = 0; t < 4; ++ t) {
		std::vector<int32_t> rows, cols;
		for(int i = 0; i < sizes[t]; ++ i) {
			const int n_kind = int(rng() % 5);
			const int32_t r = int32_t(rng() % unsigned(sets.n()));
			const int32_t c = (n_kind == 0)? r : (n_kind == 1)? int32_t(n) /* the set of every column */ :
				(n_kind == 2)? int32_t(n + rng() % unsigned(n_wide)) : int32_t(rng() % unsigned(sets.n()));
			rows.push_back(r);
			cols.push_back(c);
			if(n_kind == 4 && i + 1 < sizes[t]) { // listed twice, the second time transposed
				rows.push_back(c);
				cols.push_back(r);
				++ i;
			}
		}
		if(!check(name, P, sets, rows, cols))
			return false;
	}
	return check_single_source(name, P, rng);
}

int main()
{
	std::mt19937 rng(11);
	bool b_ok = true;
	{ // a band of half-width 3
		const int n = 400;
		CEdgeList e;
		for(int i = 0; i < n; ++ i) {
			for(int d = 1; d <= 3 && i + d < n; ++ d)
				e.push_back(std::make_pair(i, i + d));
		}
		PlanOptions opt;
		opt.dense_top_nb = 0;
		b_ok = run("band", n, e, 6, opt, rng) && b_ok;
		PlanOptions top;
		top.dense_top_nb = 3;
		top.dense_top_auto = false;
		top.dense_top_min_dim = 0;
		b_ok = run("band+dense_top", n, e, 6, top, rng) && b_ok;
	}
	{ // a star: every vertex hangs on vertex 0
		const int n = 300;
		CEdgeList e;
		for(int i = 1; i < n; ++ i)
			e.push_back(std::make_pair(0, i));
		PlanOptions opt;
		opt.dense_top_nb = 0;
		b_ok = run("star", n, e, 3, opt, rng) && b_ok;
	}
	{ // two components (a chain and a grid) and a few isolated vertices: reaches that never meet
		const int w = 12, n_chain = 200, n = n_chain + w * w + 5;
		CEdgeList e;
		for(int i = 1; i < n_chain; ++ i)
			e.push_back(std::make_pair(i - 1, i));
		const CEdgeList g = grid_graph(w);
		for(size_t i = 0; i < g.size(); ++ i)
			e.push_back(std::make_pair(n_chain + g[i].first, n_chain + g[i].second));
		PlanOptions opt;
		opt.dense_top_nb = 0;
		b_ok = run("two_components", n, e, 7, opt, rng) && b_ok;
	}
	return b_ok? 0 : 1;
}
