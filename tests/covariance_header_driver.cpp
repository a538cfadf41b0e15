// covariance_header_driver.cpp -- runs the covariance members of both solver classes of include/slam/LinearSolver_HIP.h on
// the CPU against the stand-ins for the C ABI of tests/capi_standins.h: "parts" runs Marginals with an EBlockMatrixPart and
// Marginal_Columns, "pairs" runs Marginal_Blocks and Joint_Marginal; "sparse" takes CLinearSolver_HIP, "schur"
// CLinearSolver_Schur_HIP on a BA lambda with the cameras first, one whose cameras and landmarks are interleaved (the class
// reorders it: some pairs reach the library turned around) and one without a landmark part (the class's sparse solver
// answers).  Built and run by tests/test_*covariance*_header.py against the reference's block matrix: the two words are its
// arguments (none: everything).  Prints "ok" and exits 0.
#include "capi_standins.h"

struct TSystem {
	std::vector<size_t> dims;
	TBlockSet blocks; // of lambda (upper)
	bool b_schur, b_flips; // with the Schur class: its Schur entries answer; the ordering turns some pairs around
	const char *p_s_name;
};

static TSystem t_System(const char *p_s_name, const char *p_s_dims, const size_t (*p_blocks)[2], size_t n_block_num, bool b_schur, bool b_flips)
{
	TSystem t;
	for(; *p_s_dims; ++ p_s_dims)
		t.dims.push_back(size_t(*p_s_dims - '0'));
	for(size_t c = 0; c < t.dims.size(); ++ c)
		t.blocks.insert(std::make_pair(c, c));
	for(size_t k = 0; k < n_block_num; ++ k)
		t.blocks.insert(std::make_pair(p_blocks[k][0], p_blocks[k][1]));
	t.b_schur = b_schur;
	t.b_flips = b_flips;
	t.p_s_name = p_s_name;
	return t;
}

// BA, cameras first: 3 cameras (6) with an odometry chain, 4 landmarks (3)
static const size_t cameras_first[][2] = {{0, 1}, {1, 2}, {0, 3}, {1, 3}, {1, 4}, {2, 4}, {0, 5}, {2, 5}, {2, 6}};
// BA, cameras (6) and landmarks (3) interleaved: the class reorders, the library sees the cameras first.  Landmark 1: cameras
// 0, 2; landmark 3: cameras 2, 5; landmark 4: cameras 0, 5; landmark 6: camera 5; the camera chain
static const size_t interleaved[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 5}, {0, 4}, {4, 5}, {5, 6}, {0, 2}, {2, 5}};
// no landmark part (every block column as wide): a chain with one closure; the Schur class's sparse solver answers, the same way
static const size_t chain[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {0, 3}};
// mixed block sizes: a chain plus the chords (0, 3) and (2, 5)
static const size_t mixed[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {0, 3}, {2, 5}};

// every part combination and Marginal_Columns on one lambda
template <class CSolver>
static void Check_Parts(const TSystem &r_t)
{
	const bool b_schur = r_t.b_schur;
	const std::vector<size_t> &r_dims = r_t.dims;
	const size_t n = r_dims.size();
	CUberBlockMatrix lambda;
	Make_Lambda(lambda, r_dims, r_t.blocks);
	Set_Library_Order(lambda, r_dims, b_schur);
	TBlockSet diag, last_block, last_col, full;
	for(size_t j = 0; j < n; ++ j) {
		diag.insert(std::make_pair(j, j));
		last_col.insert(std::make_pair(j, n - 1));
		for(size_t i = 0; i <= j; ++ i)
			full.insert(std::make_pair(i, j));
	}
	last_block.insert(std::make_pair(n - 1, n - 1));
	struct { int n_part; bool b_lambda; const TBlockSet *p_a, *p_b; const char *p_s_name; } cases[] = {
		{mpart_LastBlock, false, &last_block, 0, "mpart_LastBlock"},
		{mpart_LastColumn, false, &last_col, 0, "mpart_LastColumn"},
		{mpart_Diagonal, false, &diag, 0, "mpart_Diagonal"},
		{mpart_LastColumn | mpart_Diagonal, false, &last_col, &diag, "mpart_LastColumn | mpart_Diagonal"},
		{mpart_LastBlock | mpart_Diagonal, false, &last_block, &diag, "mpart_LastBlock | mpart_Diagonal"},
		{mpart_FullMatrix, false, &full, 0, "mpart_FullMatrix"},
		{mpart_FullMatrix, true, &full, 0, "mpart_FullMatrix + lambda's structure"},
		{mpart_Diagonal, true, &diag, &r_t.blocks, "mpart_Diagonal + lambda's structure"},
		{mpart_LastBlock, true, &last_block, &r_t.blocks, "mpart_LastBlock + lambda's structure"},
		{mpart_LastColumn, true, &last_col, &r_t.blocks, "mpart_LastColumn + lambda's structure"},
		{mpart_Nothing, true, &r_t.blocks, 0, "lambda's structure"}
	};
	CSolver solver;
	for(size_t t = 0; t < sizeof(cases) / sizeof(cases[0]); ++ t) {
		TBlockSet expected(*cases[t].p_a);
		if(cases[t].p_b)
			expected.insert(cases[t].p_b->begin(), cases[t].p_b->end());
		CUberBlockMatrix marginals;
		bool b_ok = false;
		const int n_calls_before = g_n_schur_calls;
		try {
			b_ok = solver.Marginals(marginals, lambda, EBlockMatrixPart(cases[t].n_part), cases[t].b_lambda);
		} catch(std::exception &r_exc) {
			fprintf(stderr, "%s, %s: %s\n", r_t.p_s_name, cases[t].p_s_name, r_exc.what());
		}
		CHECK(b_ok);
		CHECK((g_n_schur_calls > n_calls_before) == b_schur);
		if(b_ok) {
			std::string s_name = std::string(r_t.p_s_name) + ", " + cases[t].p_s_name;
			Check_Blocks(marginals, lambda, expected, s_name.c_str());
		}
	}
	// mpart_Column does not say which column: refused, alone and in a union
	const int column_parts[] = {mpart_Column, mpart_Column | mpart_Diagonal, mpart_Column | mpart_LastColumn};
	for(size_t t = 0; t < 3; ++ t) {
		CUberBlockMatrix marginals;
		bool b_thrown = false;
		try {
			solver.Marginals(marginals, lambda, EBlockMatrixPart(column_parts[t]));
		} catch(std::runtime_error&) {
			b_thrown = true;
		}
		CHECK(b_thrown);
	}
	// Marginal_Columns: n_scalars x k, the listed columns in order, rows in lambda's scalar order
	std::vector<size_t> cols;
	cols.push_back(n - 2);
	cols.push_back(0);
	cols.push_back(1);
	Eigen::MatrixXd X;
	CHECK(solver.Marginal_Columns(X, lambda, cols));
	size_t n_k = 0;
	for(size_t q = 0; q < cols.size(); ++ q)
		n_k += r_dims[cols[q]];
	CHECK(size_t(X.rows()) == lambda.n_Column_Num() && size_t(X.cols()) == n_k);
	for(size_t q = 0, c = 0; q < cols.size() && size_t(X.cols()) == n_k; ++ q) {
		for(size_t d = 0; d < r_dims[cols[q]]; ++ d, ++ c) {
			const int64_t s = int64_t(lambda.n_BlockColumn_Base(cols[q]) + d);
			for(int r = 0; r < X.rows(); ++ r)
				CHECK(X(r, int(c)) == S(r, s));
		}
	}
	bool b_thrown = false;
	try {
		std::vector<size_t> bad(1, n);
		solver.Marginal_Columns(X, lambda, bad);
	} catch(std::runtime_error&) {
		b_thrown = true;
	}
	CHECK(b_thrown);
}

// Marginal_Blocks at every ordered pair of block columns (r > c and pairs outside lambda's pattern among them) and one
// listed twice, and Joint_Marginal of a mixed set, on one lambda
template <class CSolver>
static void Check_Pairs(const TSystem &r_t)
{
	const bool b_schur = r_t.b_schur, b_flips = r_t.b_flips;
	const std::vector<size_t> &r_dims = r_t.dims;
	const size_t n = r_dims.size();
	CUberBlockMatrix lambda;
	Make_Lambda(lambda, r_dims, r_t.blocks);
	Set_Library_Order(lambda, r_dims, b_schur);
	CSolver solver;
	std::vector<std::pair<size_t, size_t> > pairs;
	for(size_t r = 0; r < n; ++ r)
		for(size_t c = 0; c < n; ++ c)
			pairs.push_back(std::make_pair(r, c));
	pairs.push_back(std::make_pair(size_t(1), n - 1)); // listed twice
	std::vector<Eigen::MatrixXd> blocks;
	const int n_calls_before = g_n_schur_calls, n_flipped_before = g_n_flipped;
	bool b_ok = false;
	try {
		b_ok = solver.Marginal_Blocks(blocks, lambda, pairs);
	} catch(std::exception &r_exc) {
		fprintf(stderr, "%s: Marginal_Blocks: %s\n", r_t.p_s_name, r_exc.what());
	}
	CHECK(b_ok && blocks.size() == pairs.size());
	CHECK((g_n_schur_calls > n_calls_before) == b_schur);
	CHECK((g_n_flipped > n_flipped_before) == b_flips);
	for(size_t k = 0; b_ok && k < blocks.size(); ++ k) { // block (r, c) of lambda's own order, whatever the library's order is
		const size_t r0 = lambda.n_BlockColumn_Base(pairs[k].first), c0 = lambda.n_BlockColumn_Base(pairs[k].second);
		CHECK(size_t(blocks[k].rows()) == r_dims[pairs[k].first] && size_t(blocks[k].cols()) == r_dims[pairs[k].second]);
		for(int c = 0; c < blocks[k].cols(); ++ c)
			for(int r = 0; r < blocks[k].rows(); ++ r)
				CHECK(blocks[k](r, c) == S(int64_t(r0 + r), int64_t(c0 + c)));
	}
	// Joint_Marginal: the listed columns in the listed order
	std::vector<size_t> cols;
	cols.push_back(n - 1); cols.push_back(0); cols.push_back(n - 2); cols.push_back(1);
	std::vector<int64_t> scalars;
	for(size_t q = 0; q < cols.size(); ++ q)
		for(size_t d = 0; d < r_dims[cols[q]]; ++ d)
			scalars.push_back(int64_t(lambda.n_BlockColumn_Base(cols[q]) + d));
	Eigen::MatrixXd joint;
	CHECK(solver.Joint_Marginal(joint, lambda, cols));
	CHECK(size_t(joint.rows()) == scalars.size() && size_t(joint.cols()) == scalars.size());
	for(size_t c = 0; c < scalars.size() && size_t(joint.cols()) == scalars.size(); ++ c)
		for(size_t r = 0; r < scalars.size(); ++ r)
			CHECK(joint(int(r), int(c)) == S(scalars[r], scalars[c]));
	// refusals: an index out of range, a column listed twice, an empty set
	const size_t bad_cols[][2] = {{0, n}, {1, 1}};
	for(size_t t = 0; t < 3; ++ t) {
		bool b_thrown = false;
		try {
			std::vector<size_t> bad;
			if(t < 2)
				bad.assign(bad_cols[t], bad_cols[t] + 2);
			solver.Joint_Marginal(joint, lambda, bad);
		} catch(std::runtime_error&) {
			b_thrown = true;
		}
		CHECK(b_thrown);
	}
	bool b_thrown = false;
	try {
		std::vector<std::pair<size_t, size_t> > bad(1, std::make_pair(n, size_t(0)));
		solver.Marginal_Blocks(blocks, lambda, bad);
	} catch(std::runtime_error&) {
		b_thrown = true;
	}
	CHECK(b_thrown);
}

int main(int n_arg_num, const char **p_arg_list)
{
	const std::string s_class = (n_arg_num == 3)? p_arg_list[1] : "both", s_what = (n_arg_num == 3)? p_arg_list[2] : "all";
	if((n_arg_num != 1 && n_arg_num != 3) || (s_class != "sparse" && s_class != "schur" && s_class != "both") ||
	   (s_what != "parts" && s_what != "pairs" && s_what != "all")) {
		fprintf(stderr, "use: covariance_header_driver [sparse|schur parts|pairs]\n");
		return 2;
	}
	const bool b_parts = s_what != "pairs", b_pairs = s_what != "parts";
	std::vector<TSystem> systems;
	systems.push_back(t_System("cameras first", "6663333", cameras_first, 9, true, false));
	systems.push_back(t_System("interleaved", "6363363", interleaved, 9, true, true));
	systems.push_back(t_System("no landmark part", "66666", chain, 5, false, false));
	for(size_t i = 0; s_class != "sparse" && i < systems.size(); ++ i) {
		if(b_parts)
			Check_Parts<CLinearSolver_Schur_HIP<> >(systems[i]);
		if(b_pairs)
			Check_Pairs<CLinearSolver_Schur_HIP<> >(systems[i]);
	}
	if(s_class != "schur") { // (the sparse class takes lambda as it is: no Schur entry answers, nothing is turned around)
		if(b_parts) {
			Check_Parts<CLinearSolver_HIP>(t_System("mixed block sizes", "323323", mixed, 7, false, false));
			Check_Parts<CLinearSolver_HIP>(systems[2]);
		}
		if(b_pairs)
			Check_Pairs<CLinearSolver_HIP>(systems[2]);
	}
	if(n_failures) {
		fprintf(stderr, "%d failures\n", n_failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
