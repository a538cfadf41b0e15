/*
 * tests/robust_golden_driver.cpp -- TEST INFRASTRUCTURE: generates what tests/golden/robust/{kernels,se3_outliers}.npz hold of
 * the reference (run by tests/golden/make_robust_golden.py where the reference's headers and archives are present).
 *
 * usage: robust_golden_driver kernels <out.bin>
 *   The reference's CHuberLoss, CCauchyLoss, CTukeyBiweightLoss and CWelschLoss operator (), each at its default parameter and
 *   at a = 1, on the grid s = 0, a / 2, the double below a, a, the double above a, 2 a, 10 a, 1e3 a; then
 *   CRobustify_ErrorNorm_Default<CCTFraction<30, 100>, CHuberLossd>::f_RobustWeight on n_vectors 6-vectors.
 *   out: for kernel = Huber, Cauchy, Tukey, Welsch, for the two parameters: double a, then n_grid times (s, w);
 *        then n_vectors times (v[6], w)
 *
 * usage: robust_golden_driver lm <in.bin> <out.bin> <f_min_dx_norm>
 *   The SE(3) graph of the input file (that of tests/lm_golden_driver.cpp, kind 2) in the reference's CVertexPose3D and
 *   CEdgePose3D -- a robust edge: Huber on |err| / 0.3 -- and the reference's CNonlinearSolver_Lambda_LM on it, unchanged:
 *   Optimize(n_max, f_min_dx_norm) for n_max = 1 .. 8, each from the same start.
 *   out: double weight[n_edges] (every edge's own f_RobustWeight of its error at the start state); unary_vertex, unary_dim,
 *        unary_factor[unary_dim^2] (column-major), unary_error[unary_dim]; then for n_max = 1 .. 8: double chi2, n_iterations,
 *        state[n_scalars]
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>

#include "slam/LinearSolver_CholMod.h"
#include "slam/ConfigSolvers.h"
#include "slam/SE3_Types.h"
#include "slam/NonlinearSolver_Lambda_LM.h"
#include "geometry/RobustLoss.h"
#include "slam/RobustUtils.h"

enum { n_max_runs = 8, n_grid = 8, n_vectors = 6 };

template <class CLoss>
static void Dump_Kernel(double f_default, std::vector<double> &r_out)
{
	const double p_param[2] = { f_default, 1.0 };
	for(int i = 0; i < 2; ++ i) {
		const double a = p_param[i];
		const CLoss loss = (i)? CLoss(a) : CLoss(); // (the default parameter is the class' own: f_default says where its grid lies)
		const double p_s[n_grid] = { 0.0, a / 2, nextafter(a, 0.0), a, nextafter(a, 2 * a), 2 * a, 10 * a, 1e3 * a };
		r_out.push_back(a);
		for(int j = 0; j < n_grid; ++ j) {
			r_out.push_back(p_s[j]);
			r_out.push_back(loss(p_s[j]));
		}
	}
}

static void Dump_Kernels(std::vector<double> &r_out)
{
	Dump_Kernel<CHuberLossd>(1.345, r_out);
	Dump_Kernel<CCauchyLossd>(2.385, r_out);
	Dump_Kernel<CTukeyBiweightLossd>(4.685, r_out);
	Dump_Kernel<CWelschLossd>(2.985, r_out);
	const CRobustify_ErrorNorm_Default<CCTFraction<30, 100>, CHuberLossd> robustify;
	for(int k = 0; k < n_vectors; ++ k) {
		Eigen::Matrix<double, 6, 1> v;
		for(int i = 0; i < 6; ++ i)
			v(i) = 0.045 * (k + 1) * sin(1.0 + 1.7 * i + 0.3 * k); // norms on both sides of 0.3 * 1.345
		for(int i = 0; i < 6; ++ i)
			r_out.push_back(v(i));
		r_out.push_back(robustify.f_RobustWeight(v));
	}
}

struct TInput {
	int64_t n_kind, n_verts, n_edges, n_cams;
	std::vector<double> state, z, sigma_inv;
	std::vector<int64_t> v0, v1;
};

typedef CFlatSystem<CVertexPose3D, MakeTypelist(CVertexPose3D), CEdgePose3D, MakeTypelist(CEdgePose3D)> CSystemType;

// the reference's LM solver with its iteration counter readable
class CLM_Exposed : public CNonlinearSolver_Lambda_LM<CSystemType, CLinearSolver_CholMod> {
public:
	CLM_Exposed(CSystemType &r_system)
		:CNonlinearSolver_Lambda_LM<CSystemType, CLinearSolver_CholMod>(r_system, TIncrementalSolveSetting(),
		TMarginalsComputationPolicy(), false, CLinearSolver_CholMod(), false)
	{}
	size_t n_Iteration_Num() const { return this->m_n_iteration_num; }
};

// every edge's own weight of its own error
class CDumpWeight {
	std::vector<double> *m_p_out;
public:
	CDumpWeight(std::vector<double> &r_out) :m_p_out(&r_out) {}
	void operator ()(const CEdgePose3D &r_edge)
	{
		Eigen::Matrix<double, 6, 6> J0, J1;
		Eigen::Matrix<double, 6, 1> v_exp, v_err;
		r_edge.Calculate_Jacobians_Expectation_Error(J0, J1, v_exp, v_err);
		m_p_out->push_back(r_edge.f_RobustWeight(v_err));
	}
};

static void Build(CSystemType &r_system, const TInput &in)
{
	for(int64_t v = 0; v < in.n_verts; ++ v) {
		Eigen::Matrix<double, 6, 1> v_state = Eigen::Map<const Eigen::Matrix<double, 6, 1> >(&in.state[6 * v]);
		r_system.r_Get_Vertex<CVertexPose3D>(size_t(v), v_state);
	}
	for(int64_t e = 0; e < in.n_edges; ++ e) {
		Eigen::Matrix<double, 6, 1> z = Eigen::Map<const Eigen::Matrix<double, 6, 1> >(&in.z[6 * e]);
		Eigen::Matrix<double, 6, 6> information = Eigen::Map<const Eigen::Matrix<double, 6, 6> >(&in.sigma_inv[36 * e]);
		r_system.r_Add_Edge(CEdgePose3D(size_t(in.v0[e]), size_t(in.v1[e]), z, information, r_system));
	}
}

static void Run_LM(const TInput &in, double f_min_dx_norm, std::vector<double> &r_out)
{
	for(int n_max = 1; n_max <= n_max_runs; ++ n_max) {
		CSystemType system;
		Build(system, in);
		if(n_max == 1)
			system.r_Edge_Pool().For_Each(CDumpWeight(r_out));
		CLM_Exposed solver(system);
		solver.Optimize(size_t(n_max), f_min_dx_norm);
		if(n_max == 1) {
			const Eigen::MatrixXd &r_t_uf = system.r_t_Unary_Factor();
			const Eigen::VectorXd &r_v_uerr = system.r_v_Unary_Error();
			r_out.push_back(double(system.r_Edge_Pool()[0].n_Vertex_Id(0)));
			r_out.push_back(double(r_t_uf.rows()));
			for(int c = 0; c < r_t_uf.cols(); ++ c) {
				for(int r = 0; r < r_t_uf.rows(); ++ r)
					r_out.push_back(r_t_uf(r, c));
			}
			for(int r = 0; r < r_t_uf.rows(); ++ r)
				r_out.push_back((r < r_v_uerr.rows())? r_v_uerr(r) : 0.0);
		}
		r_out.push_back(solver.f_Chi_Squared_Error_Denorm());
		r_out.push_back(double(solver.n_Iteration_Num()));
		for(size_t i = 0, n = system.r_Vertex_Pool().n_Size(); i < n; ++ i) {
			Eigen::VectorXd v = system.r_Vertex_Pool()[i].v_State();
			for(int d = 0; d < 6; ++ d)
				r_out.push_back(v(d));
		}
	}
}

template <class T>
static bool Read(FILE *f, std::vector<T> &r_v, size_t n)
{
	r_v.resize(n);
	return !n || fread(&r_v[0], sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
	std::vector<double> out;
	const char *p_s_out;
	if(argc == 3 && !strcmp(argv[1], "kernels")) {
		Dump_Kernels(out);
		p_s_out = argv[2];
	} else if(argc == 5 && !strcmp(argv[1], "lm")) {
		TInput in;
		FILE *f = fopen(argv[2], "rb");
		int64_t hdr[4];
		if(!f || fread(hdr, 8, 4, f) != 4)
			return 1;
		in.n_kind = hdr[0]; in.n_verts = hdr[1]; in.n_edges = hdr[2]; in.n_cams = hdr[3];
		if(in.n_kind != 2)
			return 2;
		if(!Read(f, in.state, 6 * in.n_verts) || !Read(f, in.v0, in.n_edges) || !Read(f, in.v1, in.n_edges) ||
		   !Read(f, in.z, in.n_edges * 6) || !Read(f, in.sigma_inv, in.n_edges * 36))
			return 1;
		fclose(f);
		Run_LM(in, atof(argv[4]), out);
		p_s_out = argv[3];
	} else
		return 2;
	FILE *f = fopen(p_s_out, "wb");
	if(!f)
		return 1;
	fwrite(&out[0], sizeof(double), out.size(), f);
	fclose(f);
	printf("ok\n");
	return 0;
}
