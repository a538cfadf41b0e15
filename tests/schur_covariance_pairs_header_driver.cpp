// schur_covariance_pairs_header_driver.cpp -- runs Marginal_Blocks and Joint_Marginal of CLinearSolver_Schur_HIP
// (include/slam/LinearSolver_HIP.h) on the CPU against stand-ins for the C ABI.  The stand-ins answer every pair with the block
// of a known symmetric matrix S(r, c) of lambda's scalars, seen through the guided ordering the class hands the library, so
// the driver checks that the caller gets block (r, c) of lambda's own order -- for a BA lambda with the cameras first, one
// whose cameras and landmarks are interleaved (the class reorders it: some pairs reach the library turned around), and one
// without a landmark part (the class's sparse solver answers).  Built and run by
// tests/test_schur_covariance_pairs_header.py against the reference's block matrix.  Prints "ok" and exits 0.
#include "slam/LinearSolver_HIP.h"
#include <cmath>
#include <set>

// ---- stand-ins for the C ABI (what the header calls) ----

struct slampp_hip_solver {
	std::vector<int64_t> cumsum, bcol_ptr;
	std::vector<int32_t> brow;
	std::vector<double> values, rhs;
};

static double S(int64_t r, int64_t c) // the "covariance": symmetric, every entry distinct (lambda's scalar indices)
{
	const int64_t a = std::min(r, c), b = std::max(r, c);
	return double(a) * 1009 + double(b) + 0.25;
}

// the library sees lambda in the Schur class's guided order: its scalar s is lambda's scalar g_lambda_scalar[s] (empty: the same)
static std::vector<int64_t> g_lambda_scalar;
static int g_n_schur_calls = 0; // calls of the Schur covariance stand-ins

static double S_lib(int64_t r, int64_t c) // the covariance at the library's scalars (r, c)
{
	return (g_lambda_scalar.empty())? S(r, c) : S(g_lambda_scalar[size_t(r)], g_lambda_scalar[size_t(c)]);
}

extern "C" {
int slampp_hip_create(slampp_hip_solver **pp, int) { *pp = new slampp_hip_solver(); return SLAMPP_HIP_OK; }
int slampp_hip_create_multi(slampp_hip_solver **pp, const int *, int) { *pp = new slampp_hip_solver(); return SLAMPP_HIP_OK; }
int slampp_hip_group_info(const slampp_hip_solver *, int *p_n, int64_t *, int, const char **) { if(p_n) *p_n = 0; return SLAMPP_HIP_OK; }
void slampp_hip_destroy(slampp_hip_solver *p) { delete p; }
const char *slampp_hip_last_error(const slampp_hip_solver *) { return "stand-in"; }
int slampp_hip_set_option(slampp_hip_solver *, const char *, int64_t) { return SLAMPP_HIP_OK; }
int slampp_hip_set_structure(slampp_hip_solver *p, int64_t n, const int64_t *cs, const int64_t *ptr, const int32_t *brow)
{
	p->cumsum.assign(cs, cs + n + 1);
	p->bcol_ptr.assign(ptr, ptr + n + 1);
	p->brow.assign(brow, brow + ptr[n]);
	int64_t n_values = 0;
	for(int64_t c = 0; c < n; ++ c) {
		for(int64_t b = ptr[c]; b < ptr[c + 1]; ++ b)
			n_values += (cs[brow[b] + 1] - cs[brow[b]]) * (cs[c + 1] - cs[c]);
	}
	p->values.assign(size_t(n_values), 0.0);
	p->rhs.assign(size_t(cs[n]), 0.0);
	return SLAMPP_HIP_OK;
}
int slampp_hip_analyze(slampp_hip_solver *, int, int64_t) { return SLAMPP_HIP_OK; }
int slampp_hip_host_staging(slampp_hip_solver *p, double **pv, double **pr) { *pv = &p->values[0]; *pr = &p->rhs[0]; return SLAMPP_HIP_OK; }
int slampp_hip_upload_values_async(slampp_hip_solver *, int64_t, int64_t) { return SLAMPP_HIP_OK; }
int slampp_hip_factor_solve(slampp_hip_solver *, const double *, double *, slampp_hip_times *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_solve_marginal_poses(slampp_hip_solver *, const double *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_factorize(slampp_hip_solver *, const double *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_factor_structure(const slampp_hip_solver *, int64_t *, int64_t *, int64_t *, int32_t *, int32_t *, int64_t *, int32_t *,
	int64_t *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_schur_set_changed_points(slampp_hip_solver *, const int64_t *, int64_t) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_schur_marginals(slampp_hip_solver *, const double *, double *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
static int g_n_flipped = 0; // pairs r < c of lambda that reached the Schur stand-in as r' > c'

static int blocks_of_S(slampp_hip_solver *p, int64_t n_pairs, const int64_t *brows, const int64_t *bcols, double *out)
{
	const int64_t n = int64_t(p->cumsum.size()) - 1;
	if(n_pairs <= 0 || !brows || !bcols || !out)
		return SLAMPP_HIP_ERR_INVALID;
	for(int64_t k = 0; k < n_pairs; ++ k) {
		const int64_t R = brows[k], C = bcols[k];
		if(R < 0 || R >= n || C < 0 || C >= n)
			return SLAMPP_HIP_ERR_INVALID;
		for(int64_t q = p->cumsum[size_t(C)]; q < p->cumsum[size_t(C) + 1]; ++ q)
			for(int64_t r = p->cumsum[size_t(R)]; r < p->cumsum[size_t(R) + 1]; ++ r)
				*out ++ = S_lib(r, q);
	}
	return SLAMPP_HIP_OK;
}
int slampp_hip_marginal_blocks(slampp_hip_solver *p, const double *, int64_t n_pairs, const int64_t *brows, const int64_t *bcols, double *out)
{
	return blocks_of_S(p, n_pairs, brows, bcols, out);
}
int slampp_hip_schur_marginal_blocks(slampp_hip_solver *p, const double *, int64_t n_pairs, const int64_t *brows, const int64_t *bcols,
	double *out)
{
	++ g_n_schur_calls;
	for(int64_t k = 0; brows && bcols && k < n_pairs; ++ k) {
		if(!g_lambda_scalar.empty() && brows[k] >= 0 && bcols[k] >= 0 && size_t(brows[k]) + 1 < p->cumsum.size() &&
		   size_t(bcols[k]) + 1 < p->cumsum.size() && (brows[k] > bcols[k]) !=
		   (g_lambda_scalar[size_t(p->cumsum[size_t(brows[k])])] > g_lambda_scalar[size_t(p->cumsum[size_t(bcols[k])])]))
			++ g_n_flipped;
	}
	return blocks_of_S(p, n_pairs, brows, bcols, out);
}
} // extern "C"

// ---- the checks ----

static int n_failures = 0;
#define CHECK(c) do { if(!(c)) { fprintf(stderr, "failed at line %d: %s\n", __LINE__, #c); ++ n_failures; } } while(0)

typedef std::set<std::pair<size_t, size_t> > TBlockSet;

// lambda of the given block sizes with the given upper blocks (r <= c); a dominant diagonal
static void Make_Lambda(CUberBlockMatrix &r_lambda, const std::vector<size_t> &r_dims, const TBlockSet &r_blocks)
{
	for(size_t c = 0; c < r_dims.size(); ++ c) { // column by column: a block row exists before it is used further on
		for(size_t r = 0; r <= c; ++ r) {
			if(!r_blocks.count(std::make_pair(r, c)))
				continue;
				double *p = r_lambda.p_GetBlock_Log(r, c, r_dims[r], r_dims[c], true, false);
			CHECK(p != 0);
			for(size_t e = 0; p && e < r_dims[r] * r_dims[c]; ++ e)
				p[e] = (r == c && e % (r_dims[c] + 1) == 0)? 10.0 : 0.1;
		}
	}
}

// Marginal_Blocks at every ordered pair of block columns and Joint_Marginal of a mixed set on one lambda; b_schur: the Schur
// entry must have answered; b_flips: the ordering must have turned some pairs around
static void Check_System(const std::vector<size_t> &r_dims, const TBlockSet &r_lam_blocks, bool b_schur, bool b_flips, const char *p_s_system)
{
	const size_t n = r_dims.size();
	CUberBlockMatrix lambda;
	Make_Lambda(lambda, r_dims, r_lam_blocks);
	// the guided ordering the class computes (the widest block columns first, then the others, both in stable order)
	const size_t n_wide = *std::max_element(r_dims.begin(), r_dims.end());
	std::vector<size_t> order;
	for(size_t i = 0; i < n; ++ i)
		if(r_dims[i] == n_wide)
			order.push_back(i);
	for(size_t i = 0; i < n; ++ i)
		if(r_dims[i] != n_wide)
			order.push_back(i);
	g_lambda_scalar.clear();
	if(b_schur) {
		for(size_t i = 0; i < n; ++ i)
			for(size_t d = 0; d < r_dims[order[i]]; ++ d)
				g_lambda_scalar.push_back(int64_t(lambda.n_BlockColumn_Base(order[i]) + d));
	}
	CLinearSolver_Schur_HIP<> solver;
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
		fprintf(stderr, "%s: Marginal_Blocks: %s\n", p_s_system, r_exc.what());
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

int main()
{
	{ // BA, cameras first: 3 cameras (6) with an odometry chain, 4 landmarks (3)
		std::vector<size_t> dims;
		dims.push_back(6); dims.push_back(6); dims.push_back(6);
		dims.push_back(3); dims.push_back(3); dims.push_back(3); dims.push_back(3);
		TBlockSet b;
		for(size_t c = 0; c < dims.size(); ++ c)
			b.insert(std::make_pair(c, c));
		b.insert(std::make_pair(size_t(0), size_t(1))); b.insert(std::make_pair(size_t(1), size_t(2)));
		b.insert(std::make_pair(size_t(0), size_t(3))); b.insert(std::make_pair(size_t(1), size_t(3)));
		b.insert(std::make_pair(size_t(1), size_t(4))); b.insert(std::make_pair(size_t(2), size_t(4)));
		b.insert(std::make_pair(size_t(0), size_t(5))); b.insert(std::make_pair(size_t(2), size_t(5)));
		b.insert(std::make_pair(size_t(2), size_t(6)));
		Check_System(dims, b, true, false, "cameras first");
	}
	{ // BA, cameras (6) and landmarks (3) interleaved: the class reorders, the library sees the cameras first
		std::vector<size_t> dims;
		dims.push_back(6); dims.push_back(3); dims.push_back(6); dims.push_back(3);
		dims.push_back(3); dims.push_back(6); dims.push_back(3);
		TBlockSet b;
		for(size_t c = 0; c < dims.size(); ++ c)
			b.insert(std::make_pair(c, c));
		b.insert(std::make_pair(size_t(0), size_t(1))); b.insert(std::make_pair(size_t(1), size_t(2)));  // landmark 1: cameras 0, 2
		b.insert(std::make_pair(size_t(2), size_t(3))); b.insert(std::make_pair(size_t(3), size_t(5)));  // landmark 3: cameras 2, 5
		b.insert(std::make_pair(size_t(0), size_t(4))); b.insert(std::make_pair(size_t(4), size_t(5)));  // landmark 4: cameras 0, 5
		b.insert(std::make_pair(size_t(5), size_t(6)));                                                  // landmark 6: camera 5
		b.insert(std::make_pair(size_t(0), size_t(2))); b.insert(std::make_pair(size_t(2), size_t(5)));  // camera chain
		Check_System(dims, b, true, true, "interleaved");
	}
	{ // no landmark part (every block column as wide): the class's sparse solver answers, the same way
		std::vector<size_t> dims(5, 6);
		TBlockSet b;
		for(size_t c = 0; c < dims.size(); ++ c) {
			b.insert(std::make_pair(c, c));
			if(c)
				b.insert(std::make_pair(c - 1, c));
		}
		b.insert(std::make_pair(size_t(0), size_t(3)));
		Check_System(dims, b, false, false, "no landmark part");
	}
	if(n_failures) {
		fprintf(stderr, "%d failures\n", n_failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
