// Test infrastructure (tests/test_logdet_tables_host.py): the pivot table of slampp_hip_logdet (csrc/logdet_tables.cpp) on the
// graphs of tests/driver_graphs.h -- a chain with loop closures, a chain of mixed block sizes, a grid with and without a
// forced dense top, a graph in several pieces.  Every scalar pivot must be listed exactly once, in the plan's order, at
// loff(diagonal block) + i (d + 1) or at its position in the dense top; the table has as many entries as the system has
// scalars, and none of them lies in a gap or the padding of the dense top.  Built with AddressSanitizer + UBSan on the CPU.
// Prints one line per graph ("<name>: pivots .. dense .. ok") and exits 0, or says what is wrong and exits 1.
// With arguments -- <n> <cumsum..> <bcol_ptr..> <brow..> <dense_top_nb> -- it prints the table of that structure instead (one
// line "table: ..."), for the comparison with the plan the library hands to Python.
#include "logdet_tables.h"
#include "driver_graphs.h"
#include <cstdlib>
#include <cstring>
using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: column %ld: failed: %s (line %d)\n", name, long(j), #cond, __LINE__); return false; } } while(0)

static bool check(const char *name, const Plan &P)
{
	std::vector<int64_t> table;
	build_logdet_table(P, table);
	long j = -1;
	const int64_t n_scalars = P.cs_new[size_t(P.n)];
	REQUIRE(int64_t(table.size()) == n_scalars);
	const int64_t n_l_values = P.loff[P.lrow.size()];
	std::set<int64_t> seen_l, seen_dense;
	int64_t n_dense = 0;
	for(j = 0; j < P.n; ++ j) {
		const int d = P.dim[size_t(j)];
		const bool b_dense = P.dense_dim > 0 && P.dense_pos[size_t(j)] >= 0;
		REQUIRE(P.lrow[size_t(P.lptr[size_t(j)])] == j); // (the diagonal block is the first of its column)
		for(int i = 0; i < d; ++ i) {
			const int64_t e = table[size_t(P.cs_new[size_t(j)] + i)];
			if(b_dense) {
				REQUIRE(e == -(int64_t(1) + P.dense_pos[size_t(j)] + i));
				const int64_t p = -1 - e;
				REQUIRE(p >= 0 && p < P.dense_dim); // (not in the padding behind the dense top)
				REQUIRE(seen_dense.insert(p).second);
				++ n_dense;
			} else {
				const int64_t n_loff = P.loff[size_t(P.lptr[size_t(j)])];
				REQUIRE(e == n_loff + int64_t(i) * (d + 1));
				REQUIRE(e >= 0 && e < n_l_values && e < n_loff + int64_t(d) * d); // inside the diagonal block
				REQUIRE(seen_l.insert(e).second);
			}
		}
	}
	j = -1;
	REQUIRE(int64_t(seen_l.size() + seen_dense.size()) == n_scalars);
	// the positions of the dense top that no column maps to (alignment gaps) are not in the table
	std::vector<char> mapped(size_t(P.dense_dim), 0);
	for(int32_t c = 0; c < P.n; ++ c) {
		if(P.dense_dim > 0 && P.dense_pos[size_t(c)] >= 0) {
			for(int i = 0; i < P.dim[size_t(c)]; ++ i)
				mapped[size_t(P.dense_pos[size_t(c)] + i)] = 1;
		}
	}
	int64_t n_gaps = 0;
	for(int32_t p = 0; p < P.dense_dim; ++ p) {
		if(!mapped[size_t(p)]) {
			++ n_gaps;
			REQUIRE(!seen_dense.count(p));
		}
	}
	REQUIRE(n_dense + n_gaps == P.dense_dim);
	printf("%s: pivots %ld dense %ld gaps %ld ok\n", name, long(n_scalars), long(n_dense), long(n_gaps));
	return true;
}

static bool run(const char *name, int n, const CEdgeList &edges, const std::vector<int> &dims, const PlanOptions &opt)
{
	Plan P;
	return plan_of_graph(name, n, edges, dims, opt, P) && check(name, P);
}

static int print_table(int n_arg_num, char **p_arg_list)
{
	int a = 1;
	const int64_t n = atoll(p_arg_list[a ++]);
	if(n < 1 || n_arg_num < 2 + 2 * (n + 1))
		return 2;
	std::vector<int64_t> cumsum(size_t(n) + 1), ptr(size_t(n) + 1);
	for(int64_t i = 0; i <= n; ++ i)
		cumsum[size_t(i)] = atoll(p_arg_list[a ++]);
	for(int64_t i = 0; i <= n; ++ i)
		ptr[size_t(i)] = atoll(p_arg_list[a ++]);
	if(ptr[size_t(n)] < 0 || int64_t(n_arg_num) != 2 + 2 * (n + 1) + ptr[size_t(n)] + 1)
		return 2;
	const size_t n_block_num = size_t(ptr[size_t(n)]);
	std::vector<int32_t> brow(n_block_num, 0);
	for(size_t i = 0; i < brow.size(); ++ i)
		brow[i] = int32_t(atol(p_arg_list[a ++]));
	PlanOptions opt;
	const int n_dense_top_nb = atoi(p_arg_list[a ++]);
	if(n_dense_top_nb >= 0) { // (as slampp_hip_plan_create takes it: < 0 = the library default)
		opt.dense_top_nb = n_dense_top_nb;
		opt.dense_top_auto = false;
	}
	Plan P;
	const std::string err = build_plan(n, cumsum.data(), ptr.data(), brow.data(), opt, P);
	if(!err.empty()) {
		printf("build_plan: %s\n", err.c_str());
		return 1;
	}
	std::vector<int64_t> table;
	build_logdet_table(P, table);
	printf("table:");
	for(size_t i = 0; i < table.size(); ++ i)
		printf(" %ld", long(table[i]));
	printf("\n");
	return 0;
}

int main(int n_arg_num, char **p_arg_list)
{
	if(n_arg_num > 1)
		return print_table(n_arg_num, p_arg_list);
	std::mt19937 rng(7);
	bool b_ok = true;
	{
		int n = 6000;
		const CEdgeList e = chain_with_closures(n, rng);
		b_ok = run("chain", n, e, std::vector<int>(1, 6), PlanOptions()) && b_ok;
		const int mixed[] = {2, 3, 6, 7, 8, 4, 5};
		PlanOptions opt;
		opt.dense_top_nb = 0;
		b_ok = run("mixed", 900, CEdgeList(e.begin(), e.begin() + 899), std::vector<int>(mixed, mixed + 7), opt) && b_ok;
	}
	{
		int w = 40, n = w * w;
		const CEdgeList e = grid_graph(w);
		PlanOptions opt;
		opt.dense_top_nb = 0;
		b_ok = run("grid", n, e, std::vector<int>(1, 3), opt) && b_ok;
		opt.dense_top_auto = false;
		opt.dense_top_min_dim = 0;
		opt.dense_top_nb = 4; // nearly everything in the top, one chain
		b_ok = run("grid+dense_top", n, e, std::vector<int>(1, 3), opt) && b_ok;
		opt.dense_top_nb = 16; // its biggest separators only, 7 wide: chains of a tile and more side by side, aligned (gaps)
		b_ok = run("grid7+dense_top", n, e, std::vector<int>(1, 7), opt) && b_ok;
		opt.dense_top_align = 0; // the same, packed: no gaps
		b_ok = run("grid7+dense_top_packed", n, e, std::vector<int>(1, 7), opt) && b_ok;
	}
	{
		const CEdgeList e = pieces_graph(rng);
		b_ok = run("pieces", 1500, e, std::vector<int>(1, 6), PlanOptions()) && b_ok;
	}
	return b_ok? 0 : 1;
}
