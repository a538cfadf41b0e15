/*
 * tests/landmark_math_driver.cpp -- runs the arithmetic of the pose-landmark and stereo edges of the linearize kernel
 * (slam_plus_plus_amd/csrc/linearize_math.h, which compiles for the host as well) on the CPU, one edge at a time, so that the
 * suite checks it against the exact model without a GPU (tests/test_landmark_math_host.py), also under sanitizers.
 *
 * usage: landmark_math_driver <in.bin> <out.bin>
 *   in:  the input of tests/landmark_golden_driver.cpp: int64 kind (5 pose-landmark 2D, 6 pose-landmark 3D, 7 stereo), n_verts,
 *        n_edges, n_first_pose, n_poses; double state[n_scalars]; int64 v0[n_edges] (the pose), v1[n_edges];
 *        double z[n_edges * rd]; double sigma_inv[n_edges * rd * rd] (not used); double params[n_poses * 6] (stereo);
 *        double dx[n_scalars] (not used)
 *   out: double J0[n_edges * rd * d0], J1[n_edges * rd * d1] (column-major per edge), err[n_edges * rd]
 */
#include <stdio.h>
#include <stdint.h>
#include <vector>

#include "linearize_math.h"

using namespace slampp::lin;

template <class T>
static bool Read(FILE *f, std::vector<T> &r_v, size_t n)
{
	r_v.resize(n);
	return !n || fread(&r_v[0], sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
	if(argc != 3)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	int64_t hdr[5];
	if(!f || fread(hdr, 8, 5, f) != 5)
		return 1;
	const int64_t n_kind = hdr[0], n_verts = hdr[1], n_edges = hdr[2], n_first_pose = hdr[3], n_poses = hdr[4];
	if(n_kind < 5 || n_kind > 7 || n_verts < 0 || n_edges < 0 || n_first_pose < 0 || n_poses < 0 || n_first_pose + n_poses > n_verts)
		return 2;
	const int rd = (n_kind == 5)? 2 : 3, d0 = (n_kind == 5)? 3 : 6, d1 = (n_kind == 5)? 2 : 3;
	std::vector<int64_t> off(n_verts + 1, 0), v0, v1;
	for(int64_t v = 0; v < n_verts; ++ v)
		off[v + 1] = off[v] + ((v >= n_first_pose && v < n_first_pose + n_poses)? d0 : d1);
	const size_t n_scalars = size_t(off[n_verts]);
	std::vector<double> state, z, sigma_inv, params, dx;
	if(!Read(f, state, n_scalars) || !Read(f, v0, n_edges) || !Read(f, v1, n_edges) || !Read(f, z, n_edges * rd) ||
	   !Read(f, sigma_inv, n_edges * rd * rd) || !Read(f, params, (n_kind == 7)? n_poses * 6 : 0) || !Read(f, dx, n_scalars))
		return 1;
	fclose(f);
	std::vector<double> J0(n_edges * rd * d0), J1(n_edges * rd * d1), err(n_edges * rd);
	for(int64_t e = 0; e < n_edges; ++ e) {
		if(v0[e] < n_first_pose || v0[e] >= n_first_pose + n_poses || v1[e] < 0 || v1[e] >= n_verts ||
		   (v1[e] >= n_first_pose && v1[e] < n_first_pose + n_poses))
			return 3; // vertex 0 is a pose, vertex 1 is not
		const double *x0 = &state[off[v0[e]]], *x1 = &state[off[v1[e]]];
		if(n_kind == 5)
			edge_pose_landmark_2d(x0, x1, &z[2 * e], &J0[6 * e], &J1[4 * e], &err[2 * e]);
		else if(n_kind == 6)
			edge_pose_landmark_3d(x0, x1, &z[3 * e], &J0[18 * e], &J1[9 * e], &err[3 * e]);
		else
			edge_p2sc_xyz(x0, x1, &z[3 * e], &params[6 * (v0[e] - n_first_pose)], &J0[18 * e], &J1[9 * e], &err[3 * e]);
	}
	f = fopen(argv[2], "wb");
	if(!f)
		return 1;
	const std::vector<double> *p_out[] = {&J0, &J1, &err};
	for(int i = 0; i < 3; ++ i) {
		if(!p_out[i]->empty())
			fwrite(&(*p_out[i])[0], 8, p_out[i]->size(), f);
	}
	fclose(f);
	printf("ok\n");
	return 0;
}
