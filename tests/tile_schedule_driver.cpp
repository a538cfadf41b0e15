// Test infrastructure (tests/test_tile_schedule_host.py): the tables of the dense top's tile schedule
// (csrc/tile_schedule.cpp) for tile patterns given in a file, written out as text for the CPU replay (tests/tile_replay.py).
// Input, whitespace separated, any number of cases:
//   pattern T chunk budget  <T * T flags, column-major>
//   graph n n_blocks chunk budget  <n + 1 cumsum> <n + 1 bcol_ptr> <n_blocks brow>     (planned with default options)
#include "plan.h"
#include "tile_schedule.h"
#include <cstdio>
#include <cstring>
using namespace slampp;

static void put(const char *p_s_name, const std::vector<int> &r_v)
{
	printf("%s %zu", p_s_name, r_v.size());
	for(size_t i = 0; i < r_v.size(); ++ i)
		printf(" %d", r_v[i]);
	printf("\n");
}

static void put(const char *p_s_name, const std::vector<TTileRec4> &r_v)
{
	printf("%s %zu", p_s_name, 4 * r_v.size());
	for(size_t i = 0; i < r_v.size(); ++ i)
		printf(" %d %d %d %d", r_v[i].x, r_v[i].y, r_v[i].z, r_v[i].w);
	printf("\n");
}

int main(int argc, char **argv)
{
	FILE *f = (argc > 1)? fopen(argv[1], "r") : stdin;
	if(!f) {
		fprintf(stderr, "cannot open %s\n", argv[1]);
		return 2;
	}
	char s_kind[16];
	while(fscanf(f, "%15s", s_kind) == 1) {
		int T = 0, n_chunk = 0, n_budget = 0;
		std::vector<char> nz;
		if(!strcmp(s_kind, "pattern")) {
			if(fscanf(f, "%d %d %d", &T, &n_chunk, &n_budget) != 3 || T < 0 || T > 4096)
				return 2;
			nz.resize(size_t(T) * T);
			for(size_t i = 0; i < nz.size(); ++ i) {
				int v;
				if(fscanf(f, "%d", &v) != 1)
					return 2;
				nz[i] = char(v != 0);
			}
		} else if(!strcmp(s_kind, "graph")) {
			long long n, n_blocks;
			if(fscanf(f, "%lld %lld %d %d", &n, &n_blocks, &n_chunk, &n_budget) != 4 || n < 1 || n_blocks < 0)
				return 2;
			std::vector<int64_t> cumsum(size_t(n) + 1), ptr(size_t(n) + 1);
			std::vector<int32_t> brow(size_t(n_blocks), 0);
			long long v;
			for(size_t i = 0; i < cumsum.size(); ++ i) { if(fscanf(f, "%lld", &v) != 1) return 2; cumsum[i] = v; }
			for(size_t i = 0; i < ptr.size(); ++ i) { if(fscanf(f, "%lld", &v) != 1) return 2; ptr[i] = v; }
			for(size_t i = 0; i < brow.size(); ++ i) { if(fscanf(f, "%lld", &v) != 1) return 2; brow[i] = int32_t(v); }
			Plan P;
			const std::string s_err = build_plan(n, cumsum.data(), ptr.data(), brow.data(), PlanOptions(), P);
			if(!s_err.empty() || !P.dense_dim) {
				fprintf(stderr, "graph: '%s', dense top %d\n", s_err.c_str(), P.dense_dim);
				return 3;
			}
			T = dense_top_tile_pattern(P, nz);
		} else
			return 2;
		TTileTables t;
		const bool b_ok = tile_schedule_tables(T, nz, n_chunk, n_budget, t);
		printf("case %d %d %d %d %d\n", T, n_chunk, n_budget, int(b_ok), t.n_levels);
		put("nz", std::vector<int>(nz.begin(), nz.end()));
		put("height", t.height);
		put("potrf", t.potrf);
		put("trsm", t.trsm);
		put("tgt", t.tgt);
		put("src", t.src);
		put("riders", t.riders);
		put("back_diag", t.back_diag);
		put("back_carry", t.back_carry);
		put("level_potrf_ptr", t.level_potrf_ptr);
		put("level_trsm_ptr", t.level_trsm_ptr);
		put("level_tgt_ptr", t.level_tgt_ptr);
		put("level_urgent_end", t.level_urgent_end);
		put("rider_ptr", t.rider_ptr);
		put("back_diag_ptr", t.back_diag_ptr);
		put("back_carry_ptr", t.back_carry_ptr);
		printf("end\n");
	}
	if(f != stdin)
		fclose(f);
	return 0;
}
