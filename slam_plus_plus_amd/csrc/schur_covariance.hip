// schur_covariance.hip -- covariances of a BA system beyond the block diagonal, from its Schur complement.
//   Lambda = | A  U |   S = A - U C^-1 U^T,  Z = S^-1,  W = U C^-1 (W_o = U_o C_p^-1 per observation o of landmark p)
//            | U' C |
//   Lambda^-1 = | Z          -Z W            |
//               | -W^T Z     C^-1 + W^T Z W  |
// Pattern (Lambda^-1 at every stored upper block of Lambda):
//   camera blocks (a, b) of A           Z(a, b)
//   observation (c, p)                  -T_c,  T_a = sum over the cameras b observing p of Z(a, b) W_b
//   landmark diagonal p                 C_p^-1 + sum over the cameras a observing p of W_a^T T_a
// so one pass over the k^2 camera pairs of a landmark gives its k cross-covariances and its diagonal block.
// Columns: the camera part X of a pass (Z E_c for a camera column, -Z W E_p for a landmark column) comes from the dense
// inverse or from k-column substitutions with the reduced system's sparse factor (covariance.hip); the landmark rows
// are then -W_q^T X(cams(q)) per landmark q, plus C_p^-1 on a landmark column's own block.
// Z is read either from the dense inverse (dense_inverse.hip: lower triangle and diagonal 64 x 64 tiles valid, element
// (i, j) read as (max, min)) or from the sparse inverse subset on the reduced system's factor pattern (sparse_inverse.hip:
// where a block sits and whether it is stored transposed comes from host-built tables, schur_setup.hip).
// This file holds the kernels, their launches (functions of the state, one dispatch on the block sizes each) and the three
// entry points that drive them behind the reduced system's factorization: schur_cov_pattern_enqueue, schur_cov_columns_enqueue,
// schur_cov_pairs_enqueue.
#include "schur_state.h"
#include "covariance.h"
#include "pair_plan.h"

#include <algorithm>

namespace slampp {

// N contiguous doubles, 16-byte loads where the address allows it
template <int N>
__device__ __forceinline__ void cov_load(double (&r_dst)[N], const double *__restrict__ p_src)
{
	typedef double v2f64 __attribute__((ext_vector_type(2)));
	if((reinterpret_cast<uintptr_t>(p_src) & 15) == 0) {
		#pragma unroll
		for(int i = 0; i + 1 < N; i += 2) {
			const v2f64 v = *reinterpret_cast<const v2f64*>(p_src + i);
			r_dst[i] = v.x;
			r_dst[i + 1] = v.y;
		}
		if(N & 1)
			r_dst[N - 1] = p_src[N - 1];
	} else {
		#pragma unroll
		for(int i = 0; i < N; ++ i)
			r_dst[i] = p_src[i];
	}
}

// t += Z(a, b) w, Z(a, b)[r, q] = p_z[r + q * n_cs] (stored as it is) or p_z[q + r * n_cs] (stored transposed); the loads
// are contiguous runs of DC either way
template <int DC, int DP>
__device__ __forceinline__ void cov_zw_acc(double (&t)[DC * DP], const double *__restrict__ p_z, int64_t n_cs, bool b_tr,
	const double (&w)[DC * DP])
{
	if(!b_tr) {
		#pragma unroll
		for(int q = 0; q < DC; ++ q) {
			double zc[DC];
			cov_load<DC>(zc, p_z + q * n_cs);
			#pragma unroll
			for(int r = 0; r < DC; ++ r) {
				#pragma unroll
				for(int j = 0; j < DP; ++ j)
					t[r + j * DC] += zc[r] * w[q + j * DC];
			}
		}
	} else {
		#pragma unroll
		for(int r = 0; r < DC; ++ r) {
			double zr[DC];
			cov_load<DC>(zr, p_z + r * n_cs);
			#pragma unroll
			for(int j = 0; j < DP; ++ j) {
				double sum = 0;
				#pragma unroll
				for(int q = 0; q < DC; ++ q)
					sum += zr[q] * w[q + j * DC];
				t[r + j * DC] += sum;
			}
		}
	}
}

// t += Z(ca, cb) w with Z the dense inverse (leading dimension ld): the block below the diagonal as it is, the one above
// it from its mirror image, transposed, the diagonal block (max, min) element by element
template <int DC, int DP>
__device__ __forceinline__ void cov_zw_dense_acc(double (&t)[DC * DP], const double *__restrict__ Z, int ld, int64_t ca, int64_t cb,
	const double (&wb)[DC * DP])
{
	if(ca > cb)
		cov_zw_acc<DC, DP>(t, Z + size_t(ca * DC) + size_t(cb * DC) * ld, ld, false, wb);
	else if(ca < cb)
		cov_zw_acc<DC, DP>(t, Z + size_t(cb * DC) + size_t(ca * DC) * ld, ld, true, wb);
	else {
		#pragma unroll
		for(int q = 0; q < DC; ++ q) {
			#pragma unroll
			for(int r = 0; r < DC; ++ r) {
				const int h = (r > q)? r : q, m = (r > q)? q : r;
				const double z = Z[size_t(ca * DC + h) + size_t(ca * DC + m) * ld];
				#pragma unroll
				for(int j = 0; j < DP; ++ j)
					t[r + j * DC] += z * wb[q + j * DC];
			}
		}
	}
}

// ---- pattern: the camera blocks of A (diagonal and off-diagonal), one thread per element ----
// a_zent = 0: Z dense (leading dimension ld); else Z is the sparse inverse subset and a_zent[k] = offset * 2 + transposed of
// block k's Z(r, c)
template <int DC>
__global__ void __launch_bounds__(256)
schur_cov_cam_pattern_kernel(int64_t nc, const int64_t *__restrict__ ptr, const int32_t *__restrict__ brow,
	const int64_t *__restrict__ a_zent, const double *__restrict__ Z, int ld, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(gid >= ptr[nc] * (DC * DC))
		return;
	const int64_t k = gid / (DC * DC);
	const int e = int(gid - k * (DC * DC)), rr = e % DC, q = e / DC; // element (rr, q) of block k = Lambda^-1(r, c)
	if(a_zent) {
		const int64_t ent = a_zent[k], off = ent >> 1;
		out[gid] = (ent & 1)? Z[off + q + rr * DC] : Z[off + rr + q * DC];
		return;
	}
	int64_t lo = 0, hi = nc; // column of block k
	while(hi - lo > 1) {
		const int64_t mid = (lo + hi) >> 1;
		if(ptr[mid] <= k) lo = mid; else hi = mid;
	}
	const int64_t i = int64_t(brow[k]) * DC + rr, j = lo * DC + q;
	out[gid] = Z[size_t(i > j? i : j) + size_t(i > j? j : i) * ld];
}

// ---- pattern: the observation blocks and the diagonal block of every landmark ----
// COV_G lanes per landmark, lane l takes the observing cameras a = l, l + COV_G, ...: T_a over all k cameras b, then its
// cross-covariance block and its share of the diagonal; the group sums the shares by lane shuffles.  Lanes past k idle.
enum { COV_G = 8 };

template <int DC, int DP, bool SPARSE>
__global__ void __launch_bounds__(256)
schur_cov_point_pattern_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ brow, int64_t nc, int64_t np,
	int64_t ubase, const int64_t *__restrict__ pair_ptr, const int64_t *__restrict__ pair_tab, const double *__restrict__ W,
	const double *__restrict__ Cinv, const double *__restrict__ Z, int ld, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	const int64_t pt = gid / COV_G;
	const int l = int(gid % COV_G);
	const bool b_pt = pt < np;
	int64_t k0 = 0, k = 0, o0 = 0;
	if(b_pt) {
		k0 = ptr[nc + pt];
		k = ptr[nc + pt + 1] - k0 - 1; // the last block of the column is C_p itself
		o0 = k0 - ptr[nc] - pt;
	}
	double cov[DP * DP];
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		cov[i] = 0;
	for(int64_t a = l; a < k; a += COV_G) {
		const int64_t ca = brow[k0 + a];
		double t[DC * DP];
		#pragma unroll
		for(int i = 0; i < DC * DP; ++ i)
			t[i] = 0;
		for(int64_t b = 0; b < k; ++ b) {
			double wb[DC * DP];
			cov_load<DC * DP>(wb, W + (o0 + b) * (DC * DP));
			if(SPARSE) {
				const int64_t *tab = pair_tab + pair_ptr[pt];
				const int64_t hi = (a > b)? a : b, lo = (a > b)? b : a;
				const int64_t ent = tab[hi * (hi + 1) / 2 + lo]; // Z(cam_hi, cam_lo): offset * 2 + stored transposed
				const bool b_tr = ((ent & 1) != 0) != (a < b);
				cov_zw_acc<DC, DP>(t, Z + (ent >> 1), DC, b_tr, wb);
			} else {
				cov_zw_dense_acc<DC, DP>(t, Z, ld, ca, brow[k0 + b], wb);
			}
		}
		double *p_obs = out + ubase + (o0 + a) * (DC * DP) + pt * (DP * DP); // observation block (c_a, p), DC x DP
		#pragma unroll
		for(int i = 0; i < DC * DP; ++ i)
			p_obs[i] = -t[i];
		double wa[DC * DP];
		cov_load<DC * DP>(wa, W + (o0 + a) * (DC * DP));
		#pragma unroll
		for(int j = 0; j < DP; ++ j) {
			#pragma unroll
			for(int i = 0; i < DP; ++ i) {
				double sum = 0;
				#pragma unroll
				for(int r = 0; r < DC; ++ r)
					sum += wa[r + i * DC] * t[r + j * DC];
				cov[i + j * DP] += sum;
			}
		}
	}
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i) {
		#pragma unroll
		for(int m = COV_G / 2; m > 0; m >>= 1)
			cov[i] += __shfl_xor(cov[i], m, COV_G);
	}
	if(b_pt && l == 0) {
		double *p_diag = out + ubase + (o0 + k) * (DC * DP) + pt * (DP * DP);
		#pragma unroll
		for(int i = 0; i < DP * DP; ++ i)
			p_diag[i] = cov[i] + Cinv[pt * (DP * DP) + i];
	}
}

// ---- columns ----
// a pass's columns are described by col_src[j]: >= 0 the scalar column c * DC + s of camera c, < 0 -1 - (p * DP + s),
// scalar column s of landmark p

// dense Z: the camera part of a pass, one thread per (row i, column j); into the output (column-major, leading dimension
// n_ld, column n_col0 + j) and into X, interleaved (X[i * kp + j]) for the landmark rows
template <int DC, int DP>
__global__ void __launch_bounds__(256)
schur_cov_cols_dense_kernel(int64_t nc, const int64_t *__restrict__ ptr, const int32_t *__restrict__ brow,
	const double *__restrict__ W, const double *__restrict__ Z, int ld, const int64_t *__restrict__ col_src, int kp,
	double *X, double *out, int64_t n_ld, int64_t n_col0)
{
	const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	const int j = blockIdx.y;
	if(i >= nc * DC)
		return;
	const int64_t src = col_src[j];
	double x;
	if(src >= 0)
		x = Z[size_t(i > src? i : src) + size_t(i > src? src : i) * ld];
	else {
		const int64_t v = -1 - src, p = v / DP, s = v - p * DP;
		const int64_t k0 = ptr[nc + p], k = ptr[nc + p + 1] - k0 - 1, o0 = k0 - ptr[nc] - p;
		x = 0;
		for(int64_t a = 0; a < k; ++ a) {
			const int64_t c0 = int64_t(brow[k0 + a]) * DC;
			const double *w = W + (o0 + a) * (DC * DP) + s * DC;
			#pragma unroll
			for(int t = 0; t < DC; ++ t) {
				const int64_t jj = c0 + t;
				x -= Z[size_t(i > jj? i : jj) + size_t(i > jj? jj : i) * ld] * w[t];
			}
		}
	}
	X[i * kp + j] = x;
	out[i + (n_col0 + j) * n_ld] = x;
}

// sparse factor: the right-hand sides of a pass in the factor's permuted rows, interleaved (B was zeroed); one
// workgroup per column j
template <int DC, int DP>
__global__ void __launch_bounds__(64)
schur_cov_rhs_kernel(int64_t nc, const int64_t *__restrict__ ptr, const int32_t *__restrict__ brow, const double *__restrict__ W,
	const int64_t *__restrict__ cam_csn, const int64_t *__restrict__ col_src, int kp, double *B)
{
	const int j = blockIdx.x;
	const int64_t src = col_src[j];
	if(src >= 0) {
		if(threadIdx.x == 0) {
			const int64_t c = src / DC;
			B[(cam_csn[c] + (src - c * DC)) * kp + j] = 1.0;
		}
		return;
	}
	const int64_t v = -1 - src, p = v / DP, s = v - p * DP;
	const int64_t k0 = ptr[nc + p], k = ptr[nc + p + 1] - k0 - 1, o0 = k0 - ptr[nc] - p;
	for(int64_t e = threadIdx.x; e < k * DC; e += blockDim.x) {
		const int64_t a = e / DC, t = e - a * DC;
		B[(cam_csn[brow[k0 + a]] + t) * kp + j] = -W[(o0 + a) * (DC * DP) + t + s * DC];
	}
}

// the camera part of a pass as the substitutions left it in the output, interleaved into X
__global__ void __launch_bounds__(256)
schur_cov_interleave_kernel(int64_t n_rows, int kp, const double *__restrict__ out, int64_t n_ld, int64_t n_col0, double *X)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(gid >= n_rows * kp)
		return;
	const int64_t i = gid / kp;
	const int j = int(gid - i * kp);
	X[gid] = out[i + (n_col0 + j) * n_ld];
}

// the landmark rows of a pass: n_g lanes per landmark q (the power of two from kp up), lane j = column j -- a wave takes
// 64 / n_g landmarks, so a pass of one block column does not leave most of a wave idle; the W blocks are the same address
// for the lanes of a landmark, the camera rows of X are read as contiguous runs of kp doubles
template <int DC, int DP>
__global__ void __launch_bounds__(256)
schur_cov_point_rows_kernel(int64_t nc, int64_t np, const int64_t *__restrict__ ptr, const int32_t *__restrict__ brow,
	const double *__restrict__ W, const double *__restrict__ Cinv, const int64_t *__restrict__ col_src, int kp, int n_g,
	const double *__restrict__ X, double *out, int64_t n_ld, int64_t n_col0)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	const int64_t q = gid / n_g;
	const int j = int(gid % n_g);
	if(q >= np || j >= kp)
		return;
	const int64_t k0 = ptr[nc + q], k = ptr[nc + q + 1] - k0 - 1, o0 = k0 - ptr[nc] - q;
	double acc[DP];
	#pragma unroll
	for(int r = 0; r < DP; ++ r)
		acc[r] = 0;
	for(int64_t a = 0; a < k; ++ a) {
		const int64_t c0 = int64_t(brow[k0 + a]) * DC;
		double w[DC * DP], x[DC];
		cov_load<DC * DP>(w, W + (o0 + a) * (DC * DP));
		#pragma unroll
		for(int t = 0; t < DC; ++ t)
			x[t] = X[(c0 + t) * kp + j];
		#pragma unroll
		for(int r = 0; r < DP; ++ r) {
			#pragma unroll
			for(int t = 0; t < DC; ++ t)
				acc[r] -= w[t + r * DC] * x[t];
		}
	}
	const int64_t src = col_src[j];
	if(src < 0) {
		const int64_t v = -1 - src, p = v / DP, s = v - p * DP;
		if(p == q) {
			#pragma unroll
			for(int r = 0; r < DP; ++ r)
				acc[r] += Cinv[q * (DP * DP) + r + s * DP];
		}
	}
	double *p_out = out + nc * DC + q * DP + (n_col0 + j) * n_ld;
	#pragma unroll
	for(int r = 0; r < DP; ++ r)
		p_out[r] = acc[r];
}

// ---- blocks at arbitrary pairs ----
// Lambda^-1(r, c) for r <= c (TSchurPairRec; the caller's (c, r) is the same block written transposed: exact twins):
//   camera a, camera b        Z(a, b)
//   camera a, landmark q      -sum over b in cams(q) of Z(a, b) W_{b,q}
//   landmark p, landmark q    delta_pq C_p^-1 + sum over a in cams(p), b in cams(q) of W_{a,p}^T Z(a, b) W_{b,q}

enum { COV_PAIR_WAVES = 4 };

// C_p^-1 read as its upper triangle mirrored: a diagonal block comes out symmetric bit for bit
template <int DP>
__device__ __forceinline__ double cov_cinv_sym(const double *__restrict__ Cinv, int64_t p, int i, int j)
{
	return Cinv[p * (DP * DP) + ((i < j)? i : j) + ((i < j)? j : i) * DP];
}

// dense Z: one workgroup of COV_PAIR_WAVES waves per pair.  The lanes stride over the k_r k_c camera pairs (a, b) behind the
// two columns (k = 1 for a camera), each adding its terms into a block of its own; the blocks meet by a butterfly of lane
// shuffles inside a wave and through LDS across the waves, summed in wave order: no atomics, every entry in one fixed order.
template <int DC, int DP>
__global__ void __launch_bounds__(64 * COV_PAIR_WAVES)
schur_cov_pairs_dense_kernel(const TSchurPairRec *__restrict__ recs, int64_t nc, const int64_t *__restrict__ ptr,
	const int32_t *__restrict__ brow, const double *__restrict__ W, const double *__restrict__ Cinv, const double *__restrict__ Z,
	int ld, double *__restrict__ out)
{
	constexpr int NA = DC * DP; // (the largest block with a landmark in it; DP x DP uses the first DP * DP)
	__shared__ double s_part[COV_PAIR_WAVES][NA];
	const TSchurPairRec rec = recs[blockIdx.x];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	if(rec.kind == 0) { // two cameras: a gather, element (i, j) read as (max, min) of the inverse
		if(tid < DC * DC) {
			const int i = tid % DC, j = tid / DC;
			const int64_t gi = int64_t(rec.r) * DC + i, gj = int64_t(rec.c) * DC + j;
			const double z = Z[size_t(gi > gj? gi : gj) + size_t(gi > gj? gj : gi) * ld];
			out[rec.out + (rec.b_tr? j + i * DC : tid)] = z;
		}
		return;
	}
	const bool b_ll = rec.kind == 3;
	// the cameras behind the row (one camera, or those of landmark r) and behind the column (those of landmark c)
	const int64_t kr0 = b_ll? ptr[nc + rec.r] : 0, kr = b_ll? ptr[nc + rec.r + 1] - kr0 - 1 : 1, or0 = kr0 - ptr[nc] - rec.r;
	const int64_t kc0 = ptr[nc + rec.c], kc = ptr[nc + rec.c + 1] - kc0 - 1, oc0 = kc0 - ptr[nc] - rec.c;
	double acc[NA];
	#pragma unroll
	for(int i = 0; i < NA; ++ i)
		acc[i] = 0;
	for(int64_t e = tid; e < kr * kc; e += 64 * COV_PAIR_WAVES) {
		const int64_t a = e / kc, b = e - a * kc;
		const int64_t ca = b_ll? int64_t(brow[kr0 + a]) : int64_t(rec.r), cb = brow[kc0 + b];
		double wb[NA];
		cov_load<NA>(wb, W + (oc0 + b) * NA);
		if(!b_ll)
			cov_zw_dense_acc<DC, DP>(acc, Z, ld, ca, cb, wb); // (negated at the end)
		else {
			double t[NA], wa[NA];
			#pragma unroll
			for(int i = 0; i < NA; ++ i)
				t[i] = 0;
			cov_zw_dense_acc<DC, DP>(t, Z, ld, ca, cb, wb);
			cov_load<NA>(wa, W + (or0 + a) * NA);
			#pragma unroll
			for(int j = 0; j < DP; ++ j) {
				#pragma unroll
				for(int i = 0; i < DP; ++ i) {
					double sum = 0;
					#pragma unroll
					for(int r = 0; r < DC; ++ r)
						sum += wa[r + i * DC] * t[r + j * DC];
					acc[i + j * DP] += sum;
				}
			}
		}
	}
	#pragma unroll
	for(int i = 0; i < NA; ++ i) {
		#pragma unroll
		for(int m = 32; m > 0; m >>= 1)
			acc[i] += __shfl_xor(acc[i], m, 64);
	}
	if(lane == 0) {
		#pragma unroll
		for(int i = 0; i < NA; ++ i)
			s_part[w][i] = acc[i];
	}
	__syncthreads();
	const int d1 = b_ll? DP : DC; // the block is d1 x DP
	if(tid < d1 * DP) {
		int i = tid % d1, j = tid / d1;
		const bool b_diag = b_ll && rec.r == rec.c;
		if(b_diag && i > j) { // a diagonal block: its upper triangle, mirrored
			const int t = i;
			i = j;
			j = t;
		}
		double sum = s_part[0][i + j * d1];
		#pragma unroll
		for(int v = 1; v < COV_PAIR_WAVES; ++ v)
			sum += s_part[v][i + j * d1];
		if(!b_ll)
			sum = -sum;
		else if(b_diag)
			sum += cov_cinv_sym<DP>(Cinv, rec.r, i, j);
		i = tid % d1;
		j = tid / d1;
		out[rec.out + (rec.b_tr? j + i * DP : tid)] = sum;
	}
}

// sparse factor: behind the Gram products of a pass, C_p^-1 onto the blocks of its pairs (p, p); a thread per entry
template <int DP>
__global__ void __launch_bounds__(256)
schur_cov_pairs_diag_kernel(const TSchurPairRec *__restrict__ recs, int64_t n_recs, const double *__restrict__ Cinv, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	const int64_t k = gid / (DP * DP);
	if(k >= n_recs)
		return;
	const TSchurPairRec rec = recs[k];
	if(rec.kind != 3 || rec.r != rec.c)
		return;
	const int e = int(gid - k * (DP * DP));
	out[rec.out + e] += cov_cinv_sym<DP>(Cinv, rec.r, e % DP, e / DP);
}

// ---- launches: Z is the sparse inverse subset in d_m_Zs (S.b_cov_sparse) or the dense inverse in d_m_Z ----

static void schur_cov_pattern_gather(CSchurState &S, double *out, hipStream_t stream)
{
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) {
		constexpr int DC = dc(), DP = dp();
		const int64_t ubase = S.n_ablocks * DC * DC; // (the camera blocks come first in the values: ptr[nc] blocks of DC x DC)
		const bool b_sparse = S.b_cov_sparse;
		const double *Z = b_sparse? S.d_m_Zs.p() : S.d_m_Z.p();
		const int ld = b_sparse? 0 : S.Npad;
		const int64_t *pair_ptr = b_sparse? S.d_pair_ptr.p() : 0, *pair_tab = b_sparse? S.d_pair_tab.p() : 0;
		if(ubase)
			hipLaunchKernelGGL((schur_cov_cam_pattern_kernel<DC>), dim3(unsigned((ubase + 255) / 256)), dim3(256), 0, stream,
				S.nc, S.d_ptr.p(), S.d_brow.p(), b_sparse? S.d_a_zent.p() : (const int64_t*)0, Z, ld, out);
		if(S.np) {
			const dim3 grid(unsigned((S.np * COV_G + 255) / 256));
			if(b_sparse)
				hipLaunchKernelGGL((schur_cov_point_pattern_kernel<DC, DP, true>), grid, dim3(256), 0, stream,
					S.d_ptr.p(), S.d_brow.p(), S.nc, S.np, ubase, pair_ptr, pair_tab, S.d_W.p(), S.d_Cinv.p(), Z, ld, out);
			else
				hipLaunchKernelGGL((schur_cov_point_pattern_kernel<DC, DP, false>), grid, dim3(256), 0, stream,
					S.d_ptr.p(), S.d_brow.p(), S.nc, S.np, ubase, pair_ptr, pair_tab, S.d_W.p(), S.d_Cinv.p(), Z, ld, out);
		}
	});
}

// one pass of kp scalar columns, p_cols their sources, col0 the first one's place in out (leading dimension n_ld): the
// camera part from the dense inverse, into out and d_cov_X -- or (S.b_cov_sparse) its right-hand sides into the zeroed d_cov_B
static void schur_cov_cols_cam_launch(CSchurState &S, const int64_t *p_cols, int kp, int64_t col0, double *out, int64_t n_ld,
	hipStream_t stream)
{
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) {
		constexpr int DC = dc(), DP = dp();
		if(!S.b_cov_sparse)
			hipLaunchKernelGGL((schur_cov_cols_dense_kernel<DC, DP>), dim3(unsigned((S.nc * DC + 255) / 256), unsigned(kp)), dim3(256), 0,
				stream, S.nc, S.d_ptr.p(), S.d_brow.p(), S.d_W.p(), S.d_m_Z.p(), S.Npad, p_cols, kp, S.d_cov_X.p(), out, n_ld, col0);
		else
			hipLaunchKernelGGL((schur_cov_rhs_kernel<DC, DP>), dim3(unsigned(kp)), dim3(64), 0, stream, S.nc, S.d_ptr.p(), S.d_brow.p(),
				S.d_W.p(), S.d_cam_csn.p(), p_cols, kp, S.d_cov_B.p());
	});
}

// ... the camera part as the substitutions left it in out, interleaved into d_cov_X
static void schur_cov_cols_interleave_launch(CSchurState &S, int kp, int64_t col0, const double *out, int64_t n_ld, hipStream_t stream)
{
	const int64_t n_rows = S.nc * S.DC;
	hipLaunchKernelGGL(schur_cov_interleave_kernel, dim3(unsigned((n_rows * kp + 255) / 256)), dim3(256), 0, stream,
		n_rows, kp, out, n_ld, col0, S.d_cov_X.p());
}

// ... and the landmark rows from d_cov_X
static void schur_cov_cols_point_launch(CSchurState &S, const int64_t *p_cols, int kp, int64_t col0, double *out, int64_t n_ld,
	hipStream_t stream)
{
	int n_g = 1;
	while(n_g < kp)
		n_g *= 2; // (kp <= 48: n_g <= 64)
	if(S.np)
		schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) {
			hipLaunchKernelGGL((schur_cov_point_rows_kernel<dc(), dp()>), dim3(unsigned((S.np * n_g + 255) / 256)), dim3(256), 0, stream,
				S.nc, S.np, S.d_ptr.p(), S.d_brow.p(), S.d_W.p(), S.d_Cinv.p(), p_cols, kp, n_g, S.d_cov_X.p(), out, n_ld, col0);
		});
}

// ---- the entry points ----

// C^-1, W and the factor of the reduced system from these values (A = 0: what the previous covariance call left), decided
// as schur_marginals decides (options schur_sparse, marginals_dense); b_need_z: the inverse of the reduced system too
static void schur_cov_factor(slampp_hip_solver &s, CSchurState &S, const double *A, bool b_need_z)
{
	if(A) {
		if(!S.b_reduced_decided)
			schur_setup_reduced(s, S);
		S.b_cov_z_valid = false;
		S.b_cov_sparse = S.b_reduced_sparse && s.n_marginals_dense == 0 && schur_setup_sparse_marginals(s, S);
		if(S.b_cov_sparse)
			schur_marginals_sparse_factor(s, S, A); // (no inverse until one is asked for)
		else {
			schur_marginals_dense_inverse(s, S, A); // (the columns are gathered from the dense inverse as well)
			S.b_cov_z_valid = true;
		}
	}
	if(S.b_cov_sparse) {
		schur_setup_cov_tables(s, S);
		if(b_need_z && !S.b_cov_z_valid) {
			s.Phase_Begin("marginals_inverse");
			sparse_inverse_enqueue(*S.p_sinv, S.p_inner->plan, S.p_inner->d_L.p(), S.p_inner->d_Linv.p(), S.d_m_Zs.p(), s.stream);
			s.Phase_End();
			S.b_cov_z_valid = true;
		}
	}
}

// The host tables of one call (column tables, pair records) go up in one set of uploads out of the host vectors the call
// before the previous one used: its uploads have long completed, so the host does not wait for the device.  Begin: which
// of the two sets, emptied; upload: stream-ordered behind the previous call's kernels, which read the old tables.
static int schur_cov_tables_begin(CSchurState &S)
{
	const int n_buf = (S.n_cov_call ++) & 1;
	if(S.ev_cov_cols[n_buf])
		SLAMPP_HIP_CHECK(hipEventSynchronize(S.ev_cov_cols[n_buf]));
	S.h_cov_cols[n_buf].clear();
	S.h_cov_pairs[n_buf].clear();
	return n_buf;
}

static void schur_cov_tables_upload(CSchurState &S, int n_buf, hipStream_t st)
{
	if(!S.h_cov_cols[n_buf].empty())
		S.d_cov_cols.Upload(S.h_cov_cols[n_buf], st);
	if(!S.h_cov_pairs[n_buf].empty())
		S.d_cov_pairs.Upload(S.h_cov_pairs[n_buf], st);
	if(!S.ev_cov_cols[n_buf])
		SLAMPP_HIP_CHECK(hipEventCreateWithFlags(&S.ev_cov_cols[n_buf], hipEventDisableTiming));
	SLAMPP_HIP_CHECK(hipEventRecord(S.ev_cov_cols[n_buf], st));
}

void schur_cov_pattern_enqueue(slampp_hip_solver &s, const double *p_values_dev, double *p_cov_dev)
{
	CSchurState &S = *s.p_schur;
	if(p_values_dev)
		schur_invalidate_previous(&S); // C^-1, W (and the packed reduced system) are recomputed from these values
	schur_cov_factor(s, S, p_values_dev, true);
	s.Phase_Begin("pattern_gather");
	schur_cov_pattern_gather(S, p_cov_dev, s.stream);
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// Whole block columns in passes of at most COV_K_PASS scalar columns (whole block columns each).  A pass's camera part:
// dense reduced system -- gathered from its dense inverse (computed anyway: the factor's k-column substitutions would be a
// dependent chain of tile solves per pass, the gather is one launch); sparse -- k-column substitutions with its factor
// (covariance.hip), the right-hand sides E_c for a camera column and -W E_p for a landmark column.  Then the landmark rows.
void schur_cov_columns_enqueue(slampp_hip_solver &s, const double *A, int n_cols, const int64_t *p_bcols, double *out)
{
	CSchurState &S = *s.p_schur;
	if(A)
		schur_invalidate_previous(&S);
	hipStream_t st = s.stream;
	schur_cov_factor(s, S, A, false);
	const int DC = S.DC, DP = S.DP;
	const int64_t nc = S.nc, n_ld = s.n_scalars;
	const int64_t *ptr = s.bcol_ptr.data();
	const int32_t *brow = s.brow.data();
	// the column tables of every pass, one upload out of the host vector the call before the previous one used: its upload
	// has long completed, so the host does not wait for the device here
	const int n_buf = schur_cov_tables_begin(S);
	std::vector<int64_t> &h_cols = S.h_cov_cols[n_buf];
	std::vector<int> pass_first; // first listed column of every pass
	int64_t n_pass_k = COV_K_PASS;
	for(int i = 0; i < n_cols; ++ i) {
		const int64_t c = p_bcols[i], d = (c < nc)? DC : DP;
		if(n_pass_k + d > COV_K_PASS) {
			pass_first.push_back(i);
			n_pass_k = 0;
		}
		n_pass_k += d;
		for(int64_t e = 0; e < d; ++ e)
			h_cols.push_back((c < nc)? c * DC + e : -1 - ((c - nc) * DP + e));
	}
	pass_first.push_back(n_cols);
	schur_cov_tables_upload(S, n_buf, st);
	S.d_cov_X.Alloc(size_t(nc * DC) * COV_K_PASS);
	if(S.b_cov_sparse) {
		S.d_cov_B.Alloc(size_t(nc * DC) * COV_K_PASS);
		S.p_inner->Ensure_Leaf_Inverses(); // (the substitutions multiply by inv(L_jj) of every column)
	}
	s.Phase_Begin("marginal_columns");
	std::vector<int64_t> srcs;
	int64_t col0 = 0;
	for(size_t p = 0; p + 1 < pass_first.size(); ++ p) {
		int kp = 0;
		srcs.clear();
		for(int i = pass_first[p]; i < pass_first[p + 1]; ++ i) {
			const int64_t c = p_bcols[i];
			if(c < nc) {
				kp += DC;
				srcs.push_back(c);
			} else {
				kp += DP;
				for(int64_t k = ptr[c]; k < ptr[c + 1] - 1; ++ k)
					srcs.push_back(brow[k]); // the cameras observing the landmark
			}
		}
		const int64_t *p_cols = S.d_cov_cols.p() + col0;
		if(S.b_cov_sparse) {
			std::sort(srcs.begin(), srcs.end());
			srcs.erase(std::unique(srcs.begin(), srcs.end()), srcs.end());
			SLAMPP_HIP_CHECK(hipMemsetAsync(S.d_cov_B.p(), 0, size_t(nc * DC) * kp * sizeof(double), st));
			schur_cov_cols_cam_launch(S, p_cols, kp, col0, out, n_ld, st);
			covariance_columns_rhs_enqueue(*S.p_inner, int(srcs.size()), srcs.data(), kp, S.d_cov_B.p(), out, n_ld, col0);
			schur_cov_cols_interleave_launch(S, kp, col0, out, n_ld, st);
		} else
			schur_cov_cols_cam_launch(S, p_cols, kp, col0, out, n_ld, st);
		schur_cov_cols_point_launch(S, p_cols, kp, col0, out, n_ld, st);
		col0 += kp;
	}
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// Blocks at arbitrary pairs.  Dense reduced system: one launch over the pair records, each block summed from the dense
// inverse (schur_cov_pairs_dense_kernel).  Sparse: Lambda^-1(r, c) = Y_r^T Y_c (+ C_p^-1 for r = c = landmark p) with
// Y = L^-1 P E_c for a camera column and L^-1 P (-W E_q) for a landmark column -- passes of at most COV_K_PASS right-hand
// sides (both columns of a pair in one pass), each the right-hand sides, the pruned forward substitution of the reduced
// system's factor from the cameras behind the pass's columns and the Gram products over the rows two reaches share
// (covariance.hip, pair_plan.h); no backward substitution, no inverse of the reduced system, no n_scalars x k result.
void schur_cov_pairs_enqueue(slampp_hip_solver &s, const double *A, int64_t n_pairs, const int64_t *p_brows, const int64_t *p_bcols,
	double *out)
{
	CSchurState &S = *s.p_schur;
	if(A)
		schur_invalidate_previous(&S);
	hipStream_t st = s.stream;
	schur_cov_factor(s, S, A, false);
	const int DC = S.DC, DP = S.DP;
	const int64_t nc = S.nc;
	const int64_t *ptr = s.bcol_ptr.data();
	const int32_t *brow = s.brow.data();
	const int n_buf = schur_cov_tables_begin(S);
	std::vector<TSchurPairRec> &h_pairs = S.h_cov_pairs[n_buf];
	std::vector<int64_t> &h_cols = S.h_cov_cols[n_buf];
	h_pairs.resize(size_t(n_pairs));
	int64_t n_out = 0;
	for(int64_t k = 0; k < n_pairs; ++ k) {
		const int64_t r = std::min(p_brows[k], p_bcols[k]), c = std::max(p_brows[k], p_bcols[k]);
		TSchurPairRec &rec = h_pairs[size_t(k)];
		rec.out = n_out;
		rec.r = int32_t((r < nc)? r : r - nc);
		rec.c = int32_t((c < nc)? c : c - nc);
		rec.kind = ((r < nc)? 0 : 1) | ((c < nc)? 0 : 2);
		rec.b_tr = p_brows[k] > p_bcols[k];
		n_out += int64_t((r < nc)? DC : DP) * ((c < nc)? DC : DP);
	}
	if(!S.b_cov_sparse) {
		schur_cov_tables_upload(S, n_buf, st);
		s.Phase_Begin("marginal_blocks");
		schur_dispatch(DC, DP, [&](auto dc, auto dp) {
			hipLaunchKernelGGL((schur_cov_pairs_dense_kernel<dc(), dp()>), dim3(unsigned(n_pairs)), dim3(64 * COV_PAIR_WAVES), 0, st,
				S.d_cov_pairs.p(), nc, S.d_ptr.p(), S.d_brow.p(), S.d_W.p(), S.d_Cinv.p(), S.d_m_Z.p(), S.Npad, out);
		});
		s.Phase_End();
		SLAMPP_HIP_CHECK(hipGetLastError());
		return;
	}
	// the distinct columns of the call as sets of cameras of the reduced system: a camera itself, a landmark's observers
	const Plan &P = S.p_inner->plan;
	std::vector<int64_t> ids(size_t(n_pairs) * 2);
	for(int64_t k = 0; k < n_pairs; ++ k) {
		ids[size_t(2 * k)] = p_brows[k];
		ids[size_t(2 * k + 1)] = p_bcols[k];
	}
	std::vector<int64_t> sets(ids);
	std::sort(sets.begin(), sets.end());
	sets.erase(std::unique(sets.begin(), sets.end()), sets.end());
	const int32_t n_sets = int32_t(sets.size());
	std::vector<int64_t> set_ptr(size_t(n_sets) + 1, 0);
	std::vector<int32_t> set_src, set_width(size_t(n_sets), 0), set_r(size_t(n_pairs), 0), set_c(size_t(n_pairs), 0);
	for(int32_t i = 0; i < n_sets; ++ i) {
		const int64_t c = sets[size_t(i)];
		set_width[size_t(i)] = (c < nc)? DC : DP;
		if(c < nc)
			set_src.push_back(P.pinv[size_t(c)]);
		else {
			for(int64_t k = ptr[c]; k < ptr[c + 1] - 1; ++ k)
				set_src.push_back(P.pinv[size_t(brow[k])]);
		}
		set_ptr[size_t(i) + 1] = int64_t(set_src.size());
	}
	for(int64_t k = 0; k < n_pairs; ++ k) {
		// (the row of the Gram product is the caller's row: Y_r^T Y_c and Y_c^T Y_r are exact transposes of each other)
		set_r[size_t(k)] = int32_t(std::lower_bound(sets.begin(), sets.end(), ids[size_t(2 * k)]) - sets.begin());
		set_c[size_t(k)] = int32_t(std::lower_bound(sets.begin(), sets.end(), ids[size_t(2 * k + 1)]) - sets.begin());
	}
	S.p_inner->Ensure_Leaf_Inverses(); // (the substitutions multiply by inv(L_jj) of every column)
	const PairPlan &pp = covariance_pair_sets_plan(*S.p_inner, n_pairs, set_r.data(), set_c.data(), n_sets, set_ptr.data(),
		set_src.data(), set_width.data());
	std::vector<int64_t> pass_col0(pp.passes.size(), 0); // the column tables of every pass, one after the other
	for(size_t p = 0; p < pp.passes.size(); ++ p) {
		const TPairPass &pass = pp.passes[p];
		pass_col0[p] = int64_t(h_cols.size());
		for(size_t i = 0; i < pass.cols.size(); ++ i) { // (in lane order)
			const int64_t c = sets[size_t(pass.cols[i])], d = (c < nc)? DC : DP;
			for(int64_t e = 0; e < d; ++ e)
				h_cols.push_back((c < nc)? c * DC + e : -1 - ((c - nc) * DP + e));
		}
	}
	schur_cov_tables_upload(S, n_buf, st);
	S.d_cov_B.Alloc(size_t(nc * DC) * COV_K_PASS);
	s.Phase_Begin("marginal_blocks");
	for(size_t p = 0; p < pp.passes.size(); ++ p) {
		const TPairPass &pass = pp.passes[p];
		const int kp = pass.kp;
		SLAMPP_HIP_CHECK(hipMemsetAsync(S.d_cov_B.p(), 0, size_t(nc * DC) * kp * sizeof(double), st));
		schur_dispatch(DC, DP, [&](auto dc, auto dp) {
			hipLaunchKernelGGL((schur_cov_rhs_kernel<dc(), dp()>), dim3(unsigned(kp)), dim3(64), 0, st, nc, S.d_ptr.p(), S.d_brow.p(),
				S.d_W.p(), S.d_cam_csn.p(), S.d_cov_cols.p() + pass_col0[p], kp, S.d_cov_B.p());
		});
		covariance_pair_sets_pass(*S.p_inner, p, S.d_cov_B.p(), out);
		const int64_t n_recs = pass.pair1 - pass.pair0;
		schur_dispatch(DC, DP, [&](auto, auto dp) {
			hipLaunchKernelGGL(schur_cov_pairs_diag_kernel<dp()>, dim3(unsigned((n_recs * (dp() * dp()) + 255) / 256)), dim3(256), 0, st,
				S.d_cov_pairs.p() + pass.pair0, n_recs, S.d_Cinv.p(), out);
		});
	}
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
