/*
 * tests/landmark_golden_driver.cpp -- TEST INFRASTRUCTURE: generates what tests/golden/landmark/{lm2d,lm3d,stereo}.npz hold of the
 * reference (run by tests/golden/make_landmark_golden.py where the reference's headers and archives are present).
 *
 * Builds a small graph in the reference's own vertex and edge classes (CVertexPose2D + CVertexLandmark2D / CEdgePoseLandmark2D,
 * CVertexPose3D + CVertexLandmark3D / CEdgePoseLandmark3D, CVertexSCam + CVertexXYZ / CEdgeP2SC3D) with every vertex state given
 * explicitly, and dumps, per landmark edge, what Calculate_Jacobians_Expectation_Error returns, the sum of the edges'
 * f_Chi_Squared_Error, and the states after every vertex' Operator_Plus(dx) and, from the same start, Operator_Minus(dx).  The
 * pose-pose edges of the mixed graphs are not evaluated here: tests/linearize_golden_driver.cpp covers their types.
 *
 * usage: landmark_golden_driver <in.bin> <out.bin>
 *   in:  int64 kind (5 pose-landmark 2D, 6 pose-landmark 3D, 7 stereo), n_verts, n_edges, n_first_pose, n_poses: the vertices
 *        [n_first_pose, n_first_pose + n_poses) are poses or cameras, the others landmarks or points; double state[n_scalars]
 *        in the order of the vertices; int64 v0[n_edges] (the pose), v1[n_edges]; double z[n_edges * rd];
 *        double sigma_inv[n_edges * rd * rd] (column-major); double params[n_poses * 6] (stereo; else none); double dx[n_scalars]
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
	int64_t n_kind, n_verts, n_edges, n_first_pose, n_poses;
	std::vector<double> state, z, sigma_inv, params, dx;
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

template <class CPose, int D0>
struct TPlainPose { // a pose vertex is its state
	static CPose Make(const TInput &, int64_t, const double *p_state)
	{
		return CPose(Eigen::Matrix<double, D0, 1>(Eigen::Map<const Eigen::Matrix<double, D0, 1> >(p_state)));
	}
};

struct TStereoCamera { // a stereo camera carries its six parameters behind the state
	static CVertexSCam Make(const TInput &in, int64_t n_pose, const double *p_state)
	{
		Eigen::Matrix<double, 12, 1> v;
		v.head<6>() = Eigen::Map<const Eigen::Matrix<double, 6, 1> >(p_state);
		v.tail<6>() = Eigen::Map<const Eigen::Matrix<double, 6, 1> >(&in.params[6 * n_pose]);
		return CVertexSCam(v);
	}
};

template <class CEdge>
struct TPoseFirst { // the constructor takes (pose, landmark, ...)
	template <class CZ, class CInfo, class CSystem>
	static CEdge Make(size_t n_pose, size_t n_landmark, const CZ &z, const CInfo &information, CSystem &r_system)
	{
		return CEdge(n_pose, n_landmark, z, information, r_system);
	}
};

struct TPointFirst { // CEdgeP2SC3D takes (point, camera, ...); vertex 0 of the edge is the camera
	template <class CZ, class CInfo, class CSystem>
	static CEdgeP2SC3D Make(size_t n_camera, size_t n_point, const CZ &z, const CInfo &information, CSystem &r_system)
	{
		return CEdgeP2SC3D(n_point, n_camera, z, information, r_system);
	}
};

template <class CSystem, class CPose, class CPoseMaker, class CLandmark, class CEdgeMaker, int RD, int D0, int D1>
static void Run(const TInput &in, TOutput &out)
{
	const Eigen::VectorXd dx = Eigen::Map<const Eigen::VectorXd>(&in.dx[0], in.dx.size());
	for(int n_pass = 0; n_pass < 2; ++ n_pass) {
		CSystem system;
		size_t n_off = 0;
		for(int64_t v = 0; v < in.n_verts; ++ v) {
			if(v >= in.n_first_pose && v < in.n_first_pose + in.n_poses) {
				system.template r_Get_Vertex<CPose>(size_t(v), CPoseMaker::Make(in, v - in.n_first_pose, &in.state[n_off]));
				n_off += D0;
			} else {
				system.template r_Get_Vertex<CLandmark>(size_t(v), CLandmark(Eigen::Matrix<double, D1, 1>(Eigen::Map<const Eigen::Matrix<double,
					D1, 1> >(&in.state[n_off]))));
				n_off += D1;
			}
		}
		for(int64_t e = 0; e < in.n_edges; ++ e) {
			Eigen::Matrix<double, RD, 1> z = Eigen::Map<const Eigen::Matrix<double, RD, 1> >(&in.z[RD * e]);
			Eigen::Matrix<double, RD, RD> information = Eigen::Map<const Eigen::Matrix<double, RD, RD> >(&in.sigma_inv[RD * RD * e]);
			system.r_Add_Edge(CEdgeMaker::Make(size_t(in.v0[e]), size_t(in.v1[e]), z, information, system));
		}
		if(!n_pass) {
			out.f_chi2 = 0;
			system.r_Edge_Pool().For_Each(CDumpEdge<RD, D0, D1>(out));
		}
		system.r_Vertex_Pool().For_Each(CMoveVertex(dx, n_pass == 1, (n_pass)? out.state_minus : out.state_plus));
	}
}

typedef CFlatSystem<CBaseVertex, MakeTypelist_Safe((CVertexPose2D, CVertexLandmark2D)), CEdgePoseLandmark2D,
	MakeTypelist_Safe((CEdgePoseLandmark2D))> TSystem2D;
typedef CFlatSystem<CBaseVertex, MakeTypelist_Safe((CVertexPose3D, CVertexLandmark3D)), CEdgePoseLandmark3D,
	MakeTypelist_Safe((CEdgePoseLandmark3D))> TSystem3D;
typedef CFlatSystem<CBaseVertex, MakeTypelist_Safe((CVertexSCam, CVertexXYZ)), CEdgeP2SC3D, MakeTypelist_Safe((CEdgeP2SC3D))> TSystemStereo;

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
	int64_t hdr[5];
	if(!f || fread(hdr, 8, 5, f) != 5)
		return 1;
	in.n_kind = hdr[0]; in.n_verts = hdr[1]; in.n_edges = hdr[2]; in.n_first_pose = hdr[3]; in.n_poses = hdr[4];
	if(in.n_kind < 5 || in.n_kind > 7)
		return 2;
	const int rd = (in.n_kind == 5)? 2 : 3, d0 = (in.n_kind == 5)? 3 : 6, d1 = (in.n_kind == 5)? 2 : 3;
	const size_t n_scalars = d0 * in.n_poses + d1 * (in.n_verts - in.n_poses);
	if(!Read(f, in.state, n_scalars) || !Read(f, in.v0, in.n_edges) || !Read(f, in.v1, in.n_edges) || !Read(f, in.z, in.n_edges * rd) ||
	   !Read(f, in.sigma_inv, in.n_edges * rd * rd) || !Read(f, in.params, (in.n_kind == 7)? in.n_poses * 6 : 0) || !Read(f, in.dx, n_scalars))
		return 1;
	fclose(f);
	TOutput out;
	if(in.n_kind == 5)
		Run<TSystem2D, CVertexPose2D, TPlainPose<CVertexPose2D, 3>, CVertexLandmark2D, TPoseFirst<CEdgePoseLandmark2D>, 2, 3, 2>(in, out);
	else if(in.n_kind == 6)
		Run<TSystem3D, CVertexPose3D, TPlainPose<CVertexPose3D, 6>, CVertexLandmark3D, TPoseFirst<CEdgePoseLandmark3D>, 3, 6, 3>(in, out);
	else
		Run<TSystemStereo, CVertexSCam, TStereoCamera, CVertexXYZ, TPointFirst, 3, 6, 3>(in, out);
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
