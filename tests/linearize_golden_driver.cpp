/*
 * tests/linearize_golden_driver.cpp -- TEST INFRASTRUCTURE: generates what tests/golden/linearize/{se2,se3,ba}.npz hold of the
 * reference (run by tests/golden/make_linearize_golden.py where the reference's headers and archives are present).
 *
 * Builds a small graph in the reference's own vertex and edge classes (CVertexPose2D / CEdgePose2D, CVertexPose3D /
 * CEdgePose3D, CVertexCam + CVertexXYZ / CEdgeP2C3D) with every vertex state given explicitly -- not initialized from the
 * edges, so the errors are not zero -- and dumps, per edge, what Calculate_Jacobians_Expectation_Error returns, the sum of the
 * edges' f_Chi_Squared_Error, and the states after every vertex' Operator_Plus(dx) and, from the same start, Operator_Minus(dx).
 *
 * usage: linearize_golden_driver <in.bin> <out.bin>
 *   in:  int64 kind (1 SE2, 2 SE3, 3 BA), n_verts, n_edges, n_cams (BA; else 0); double state[n_scalars] (BA: the cameras first);
 *        int64 v0[n_edges], v1[n_edges]; double z[n_edges * rd]; double sigma_inv[n_edges * rd * rd] (column-major);
 *        double intrinsics[n_cams * 5]; double dx[n_scalars]
 *   out: double J0[n_edges * rd * d0], J1[n_edges * rd * d1] (column-major per edge), expectation[n_edges * rd],
 *        err[n_edges * rd], chi2[1], state_plus[n_scalars], state_minus[n_scalars]
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <vector>

#include "slam/ConfigSolvers.h"
#include "slam/SE2_Types.h"
#include "slam/SE3_Types.h"
#include "slam/BA_Types.h"

struct TInput {
	int64_t n_kind, n_verts, n_edges, n_cams;
	std::vector<double> state, z, sigma_inv, intrinsics, dx;
	std::vector<int64_t> v0, v1;
};

struct TOutput {
	std::vector<double> J0, J1, expectation, err, state_plus, state_minus;
	double f_chi2;
};

template <int RD, int D0, int D1>
struct CDumpEdge {
	TOutput *m_p_out;
	CDumpEdge(TOutput &r_out) :m_p_out(&r_out) {}
	template <class CEdge>
	void operator ()(const CEdge &r_edge)
	{
		Eigen::Matrix<double, RD, D0> J0;
		Eigen::Matrix<double, RD, D1> J1;
		Eigen::Matrix<double, RD, 1> v_exp, v_err;
		r_edge.Calculate_Jacobians_Expectation_Error(J0, J1, v_exp, v_err);
		TOutput &o = *m_p_out;
		o.J0.insert(o.J0.end(), J0.data(), J0.data() + RD * D0);
		o.J1.insert(o.J1.end(), J1.data(), J1.data() + RD * D1);
		o.expectation.insert(o.expectation.end(), v_exp.data(), v_exp.data() + RD);
		o.err.insert(o.err.end(), v_err.data(), v_err.data() + RD);
		o.f_chi2 += r_edge.f_Chi_Squared_Error();
	}
};

struct CMoveVertex { // Operator_Plus or Operator_Minus, then the state
	const Eigen::VectorXd *m_p_dx;
	bool m_b_minus;
	std::vector<double> *m_p_dest;
	CMoveVertex(const Eigen::VectorXd &r_dx, bool b_minus, std::vector<double> &r_dest) :m_p_dx(&r_dx), m_b_minus(b_minus), m_p_dest(&r_dest) {}
	template <class CVertex>
	void operator ()(CVertex &r_vertex)
	{
		if(m_b_minus)
			r_vertex.Operator_Minus(*m_p_dx);
		else
			r_vertex.Operator_Plus(*m_p_dx);
		for(int i = 0; i < int(r_vertex.n_Dimension()); ++ i)
			m_p_dest->push_back(r_vertex.r_v_State()(i));
	}
};

template <class CSystem, class CVertex, class CEdge, int RD, int D0, int D1>
static void Run_Poses(const TInput &in, TOutput &out)
{
	const Eigen::VectorXd dx = Eigen::Map<const Eigen::VectorXd>(&in.dx[0], in.dx.size());
	for(int n_pass = 0; n_pass < 2; ++ n_pass) {
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
		if(!n_pass) {
			out.f_chi2 = 0;
			system.r_Edge_Pool().For_Each(CDumpEdge<RD, D0, D1>(out));
		}
		system.r_Vertex_Pool().For_Each(CMoveVertex(dx, n_pass == 1, (n_pass)? out.state_minus : out.state_plus));
	}
}

typedef CFlatSystem<CBaseVertex, MakeTypelist_Safe((CVertexCam, CVertexXYZ)), CEdgeP2C3D, MakeTypelist_Safe((CEdgeP2C3D))> TBASystem;

static void Run_BA(const TInput &in, TOutput &out)
{
	const Eigen::VectorXd dx = Eigen::Map<const Eigen::VectorXd>(&in.dx[0], in.dx.size());
	for(int n_pass = 0; n_pass < 2; ++ n_pass) {
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
		if(!n_pass) {
			out.f_chi2 = 0;
			system.r_Edge_Pool().For_Each(CDumpEdge<2, 6, 3>(out));
		}
		system.r_Vertex_Pool().For_Each(CMoveVertex(dx, n_pass == 1, (n_pass)? out.state_minus : out.state_plus));
	}
}

template <class T>
static bool Read(FILE *f, std::vector<T> &r_v, size_t n)
{
	r_v.resize(n);
	return !n || fread(&r_v[0], sizeof(T), n, f) == n;
}

static void Write(FILE *f, const std::vector<double> &r_v)
{
	if(!r_v.empty())
		fwrite(&r_v[0], sizeof(double), r_v.size(), f);
}

int main(int argc, char **argv)
{
	if(argc != 3)
		return 2;
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
	TOutput out;
	if(in.n_kind == 1) {
		typedef CFlatSystem<CVertexPose2D, MakeTypelist(CVertexPose2D), CEdgePose2D, MakeTypelist(CEdgePose2D)> CSystemType;
		Run_Poses<CSystemType, CVertexPose2D, CEdgePose2D, 3, 3, 3>(in, out);
	} else if(in.n_kind == 2) {
		typedef CFlatSystem<CVertexPose3D, MakeTypelist(CVertexPose3D), CEdgePose3D, MakeTypelist(CEdgePose3D)> CSystemType;
		Run_Poses<CSystemType, CVertexPose3D, CEdgePose3D, 6, 6, 6>(in, out);
	} else if(in.n_kind == 3)
		Run_BA(in, out);
	else
		return 2;
	if(out.state_plus.size() != n_scalars || out.state_minus.size() != n_scalars || out.err.size() != size_t(in.n_edges * rd))
		return 3;
	f = fopen(argv[2], "wb");
	if(!f)
		return 1;
	Write(f, out.J0); Write(f, out.J1); Write(f, out.expectation); Write(f, out.err);
	fwrite(&out.f_chi2, 8, 1, f);
	Write(f, out.state_plus); Write(f, out.state_minus);
	fclose(f);
	printf("ok\n");
	return 0;
}
