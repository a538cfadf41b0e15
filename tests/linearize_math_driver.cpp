/*
 * tests/linearize_math_driver.cpp -- runs the arithmetic of the linearize / state_plus kernels (slam_plus_plus_amd/csrc/
 * linearize_math.h, which compiles for the host as well) on the CPU, one edge and one vertex at a time, so that the suite
 * checks it against the exact model without a GPU (tests/test_linearize_math_host.py).
 *
 * usage: linearize_math_driver <in.bin> <out.bin>
 *   in:  the input of tests/linearize_golden_driver.cpp: int64 kind (1 SE2, 2 SE3, 3 BA), n_verts, n_edges, n_cams; double
 *        state[n_scalars] (BA: the cameras first); int64 v0[n_edges], v1[n_edges]; double z[n_edges * rd]; double
 *        sigma_inv[n_edges * rd * rd] (not used); double intrinsics[n_cams * 5]; double dx[n_scalars]
 *   out: double J0[n_edges * rd * d0], J1[n_edges * rd * d1] (column-major per edge), err[n_edges * rd],
 *        state_plus[n_scalars], state_minus[n_scalars]
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
	int64_t hdr[4];
	if(!f || fread(hdr, 8, 4, f) != 4)
		return 1;
	const int64_t n_kind = hdr[0], n_verts = hdr[1], n_edges = hdr[2], n_cams = hdr[3];
	if(n_kind < 1 || n_kind > 3)
		return 2;
	const int rd = (n_kind == 1)? 3 : (n_kind == 2)? 6 : 2, d0 = (n_kind == 1)? 3 : 6, d1 = (n_kind == 2)? 6 : 3;
	std::vector<int64_t> off(n_verts + 1, 0), v0, v1;
	for(int64_t v = 0; v < n_verts; ++ v)
		off[v + 1] = off[v] + ((n_kind == 1)? 3 : (n_kind == 2 || v < n_cams)? 6 : 3);
	const size_t n_scalars = size_t(off[n_verts]);
	std::vector<double> state, z, sigma_inv, intrinsics, dx;
	if(!Read(f, state, n_scalars) || !Read(f, v0, n_edges) || !Read(f, v1, n_edges) || !Read(f, z, n_edges * rd) ||
	   !Read(f, sigma_inv, n_edges * rd * rd) || !Read(f, intrinsics, n_cams * 5) || !Read(f, dx, n_scalars))
		return 1;
	fclose(f);
	std::vector<double> J0(n_edges * rd * d0), J1(n_edges * rd * d1), err(n_edges * rd), plus(n_scalars), minus(n_scalars);
	for(int64_t e = 0; e < n_edges; ++ e) {
		const double *x0 = &state[off[v0[e]]], *x1 = &state[off[v1[e]]];
		if(n_kind == 1)
			edge_se2(x0, x1, &z[3 * e], &J0[9 * e], &J1[9 * e], &err[3 * e]);
		else if(n_kind == 2)
			edge_se3(x0, x1, &z[6 * e], &J0[36 * e], &J1[36 * e], &err[6 * e]);
		else
			edge_p2c_xyz(x0, x1, &z[2 * e], &intrinsics[5 * v0[e]], &J0[12 * e], &J1[6 * e], &err[2 * e]);
	}
	for(int64_t v = 0; v < n_verts; ++ v) {
		const int64_t o = off[v];
		if(n_kind == 1) {
			plus_se2(&state[o], &dx[o], 1, &plus[o]);
			plus_se2(&state[o], &dx[o], -1, &minus[o]);
		} else if(n_kind == 2 || v < n_cams) {
			plus_se3(&state[o], &dx[o], 1, &plus[o]);
			plus_se3(&state[o], &dx[o], -1, &minus[o]);
		} else {
			for(int i = 0; i < 3; ++ i) {
				plus[o + i] = state[o + i] + dx[o + i];
				minus[o + i] = state[o + i] - dx[o + i];
			}
		}
	}
	f = fopen(argv[2], "wb");
	if(!f)
		return 1;
	const std::vector<double> *p_out[] = {&J0, &J1, &err, &plus, &minus};
	for(int i = 0; i < 5; ++ i)
		fwrite(&(*p_out[i])[0], 8, p_out[i]->size(), f);
	fclose(f);
	printf("ok\n");
	return 0;
}
