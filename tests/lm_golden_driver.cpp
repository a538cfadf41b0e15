/*
 * tests/lm_golden_driver.cpp -- TEST INFRASTRUCTURE: generates what tests/golden/lm/{se2,se3,ba}.npz hold of the reference
 * (run by tests/golden/make_lm_golden.py where the reference's headers and archives are present).
 *
 * Builds the graph of a tests/golden/linearize/ fixture in the reference's own vertex and edge classes, every vertex state
 * given explicitly (as tests/linearize_golden_driver.cpp does), and runs the reference's CNonlinearSolver_Lambda_LM on it,
 * unchanged, with CLinearSolver_CholMod and without the Schur complement: Optimize(n_max, f_min_dx_norm) for n_max = 1 .. 8,
 * each from the same start.  Dumps chi^2 and the states after each, the number of iterations the solver counted, and the unary
 * factor with the vertex the system put it on.
 *
 * usage: lm_golden_driver <in.bin> <out.bin> <f_min_dx_norm>
 *   in:  the input file of linearize_golden_driver (the dx at its end is not used)
 *   out: double unary_vertex, unary_dim, unary_factor[unary_dim^2] (column-major), unary_error[unary_dim]; then for
 *        n_max = 1 .. 8: double chi2, n_iterations, state[n_scalars]
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>

#include "slam/LinearSolver_CholMod.h"
#include "slam/ConfigSolvers.h"
#include "slam/SE2_Types.h"
#include "slam/SE3_Types.h"
#include "slam/BA_Types.h"
#include "slam/NonlinearSolver_Lambda_LM.h"

enum { n_max_runs = 8 };

struct TInput {
	int64_t n_kind, n_verts, n_edges, n_cams;
	std::vector<double> state, z, sigma_inv, intrinsics, dx;
	std::vector<int64_t> v0, v1;
};

// the reference's LM solver with its iteration counter readable
template <class CSystemType>
class CLM_Exposed : public CNonlinearSolver_Lambda_LM<CSystemType, CLinearSolver_CholMod> {
public:
	CLM_Exposed(CSystemType &r_system)
		:CNonlinearSolver_Lambda_LM<CSystemType, CLinearSolver_CholMod>(r_system, TIncrementalSolveSetting(),
		TMarginalsComputationPolicy(), false, CLinearSolver_CholMod(), false)
	{}
	size_t n_Iteration_Num() const { return this->m_n_iteration_num; }
};

template <class CSystem>
static void Optimize_And_Dump(CSystem &r_system, size_t n_max, double f_min_dx_norm, bool b_first, std::vector<double> &r_out)
{
	CLM_Exposed<CSystem> solver(r_system);
	solver.Optimize(n_max, f_min_dx_norm);
	if(b_first) {
		const Eigen::MatrixXd &r_t_uf = r_system.r_t_Unary_Factor();
		const Eigen::VectorXd &r_v_uerr = r_system.r_v_Unary_Error();
		r_out.push_back(double(r_system.r_Edge_Pool()[0].n_Vertex_Id(0)));
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
	for(size_t i = 0, n = r_system.r_Vertex_Pool().n_Size(); i < n; ++ i) {
		Eigen::VectorXd v = r_system.r_Vertex_Pool()[i].v_State();
		const int n_dim = int(r_system.r_Vertex_Pool()[i].n_Dimension()); // (a camera's state carries its intrinsics behind the pose)
		for(int d = 0; d < n_dim; ++ d)
			r_out.push_back(v(d));
	}
}

template <class CSystem, class CVertex, class CEdge, int RD, int D0>
static void Run_Poses(const TInput &in, double f_min_dx_norm, std::vector<double> &r_out)
{
	for(int n_max = 1; n_max <= n_max_runs; ++ n_max) {
		CSystem system;
		for(int64_t v = 0; v < in.n_verts; ++ v) {
			Eigen::Matrix<double, D0, 1> v_state = Eigen::Map<const Eigen::Matrix<double, D0, 1> >(&in.state[D0 * v]);
			system.template r_Get_Vertex<CVertex>(size_t(v), v_state);
		}
		for(int64_t e = 0; e < in.n_edges; ++ e) {
			Eigen::Matrix<double, RD, 1> z = Eigen::Map<const Eigen::Matrix<double, RD, 1> >(&in.z[RD * e]);
			Eigen::Matrix<double, RD, RD> information = Eigen::Map<const Eigen::Matrix<double, RD, RD> >(&in.sigma_inv[RD * RD * e]);
			system.r_Add_Edge(CEdge(size_t(in.v0[e]), size_t(in.v1[e]), z, information, system));
		}
		Optimize_And_Dump(system, size_t(n_max), f_min_dx_norm, n_max == 1, r_out);
	}
}

typedef CFlatSystem<CBaseVertex, MakeTypelist_Safe((CVertexCam, CVertexXYZ)), CEdgeP2C3D, MakeTypelist_Safe((CEdgeP2C3D))> TBASystem;

static void Run_BA(const TInput &in, double f_min_dx_norm, std::vector<double> &r_out)
{
	for(int n_max = 1; n_max <= n_max_runs; ++ n_max) {
		TBASystem system;
		for(int64_t c = 0; c < in.n_cams; ++ c) {
			Eigen::Matrix<double, 11, 1> v;
			v.head<6>() = Eigen::Map<const Eigen::Matrix<double, 6, 1> >(&in.state[6 * c]);
			v.tail<5>() = Eigen::Map<const Eigen::Matrix<double, 5, 1> >(&in.intrinsics[5 * c]);
			system.r_Get_Vertex<CVertexCam>(size_t(c), v);
		}
		for(int64_t p = in.n_cams; p < in.n_verts; ++ p)
			system.r_Get_Vertex<CVertexXYZ>(size_t(p), Eigen::Vector3d(Eigen::Map<const Eigen::Vector3d>(&in.state[6 * in.n_cams + 3 * (p - in.n_cams)])));
		for(int64_t e = 0; e < in.n_edges; ++ e) {
			Eigen::Vector2d z = Eigen::Map<const Eigen::Vector2d>(&in.z[2 * e]);
			Eigen::Matrix2d information = Eigen::Map<const Eigen::Matrix2d>(&in.sigma_inv[4 * e]);
			system.r_Add_Edge(CEdgeP2C3D(size_t(in.v1[e]), size_t(in.v0[e]), z, information, system)); // (xyz id, camera id, ...): vertex 0 of the edge is the camera
		}
		Optimize_And_Dump(system, size_t(n_max), f_min_dx_norm, n_max == 1, r_out);
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
	if(argc != 4)
		return 2;
	const double f_min_dx_norm = atof(argv[3]);
	TInput in;
	FILE *f = fopen(argv[1], "rb");
	int64_t hdr[4];
	if(!f || fread(hdr, 8, 4, f) != 4)
		return 1;
	in.n_kind = hdr[0]; in.n_verts = hdr[1]; in.n_edges = hdr[2]; in.n_cams = hdr[3];
	const int rd = (in.n_kind == 1)? 3 : (in.n_kind == 2)? 6 : 2;
	const size_t n_scalars = (in.n_kind == 1)? 3 * in.n_verts : (in.n_kind == 2)? 6 * in.n_verts : 6 * in.n_cams + 3 * (in.n_verts - in.n_cams);
	if(!Read(f, in.state, n_scalars) || !Read(f, in.v0, in.n_edges) || !Read(f, in.v1, in.n_edges) || !Read(f, in.z, in.n_edges * rd) ||
	   !Read(f, in.sigma_inv, in.n_edges * rd * rd) || !Read(f, in.intrinsics, in.n_cams * 5) || !Read(f, in.dx, n_scalars))
		return 1;
	fclose(f);
	std::vector<double> out;
	if(in.n_kind == 1) {
		typedef CFlatSystem<CVertexPose2D, MakeTypelist(CVertexPose2D), CEdgePose2D, MakeTypelist(CEdgePose2D)> CSystemType;
		Run_Poses<CSystemType, CVertexPose2D, CEdgePose2D, 3, 3>(in, f_min_dx_norm, out);
	} else if(in.n_kind == 2) {
		typedef CFlatSystem<CVertexPose3D, MakeTypelist(CVertexPose3D), CEdgePose3D, MakeTypelist(CEdgePose3D)> CSystemType;
		Run_Poses<CSystemType, CVertexPose3D, CEdgePose3D, 6, 6>(in, f_min_dx_norm, out);
	} else if(in.n_kind == 3)
		Run_BA(in, f_min_dx_norm, out);
	else
		return 2;
	f = fopen(argv[2], "wb");
	if(!f)
		return 1;
	fwrite(&out[0], sizeof(double), out.size(), f);
	fclose(f);
	printf("ok\n");
	return 0;
}
