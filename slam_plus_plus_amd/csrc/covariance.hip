// covariance.hip -- covariances beyond the block diagonal: the reference's CMarginals parts other than mpart_Diagonal
// (include/slam/IncrementalPolicy.h:366-372: mpart_LastBlock, mpart_Column, mpart_LastColumn, mpart_FullMatrix).
//
// Pattern gather.  The sparse inverse subset (sparse_inverse.hip) leaves Z = Lambda^-1 on the whole filled pattern of L,
// the dense top's part in the dense inverse of its Schur complement.  Lambda's pattern lies inside L's for every ordering,
// so Lambda^-1 at Lambda's stored blocks is a gather: one 16-byte record per upper block (r, c) says where block
// (max, min) of the permuted pair lives in Z, whether it is read transposed, and where the block goes in the output.
//
// Block columns.  A block column J of Lambda^-1 solves L L^T X = P E_J.  The forward substitution is pruned: the
// right-hand side is nonzero on J's rows only, so y is nonzero only on J's path to the root of the elimination tree (the
// union of the paths for several columns).  The host lists those columns per pass, stage by stage, each with the row
// entries L(j,c) whose c is on the paths too; one wave per task of a stage walks its listed columns with all k
// right-hand sides at once (lane = right-hand side), each L block loaded once for the k of them.  The backward
// substitution covers every column (x is dense), the factorization's stages in reverse, one wave per task, and scatters
// x to the caller's order as each column is finished.  With a dense top, the listed dense-top columns only subtract
// their rows' products from the right-hand side (into a buffer of their own, n_dense_pad x k); tile-by-tile k-column
// triangular solves on the top's factor and its inverted diagonal tiles follow, the backward one writing the top's x
// where the block columns below read it.
//
// Blocks at arbitrary pairs.  Lambda^-1(r, c) = Y_r^T Y_c with Y_j = L^-1 P E_j, the pruned forward substitution's result:
// no backward substitution and no n_scalars x k output.  The pairs are grouped into passes (pair_plan.cpp); a pass runs the
// forward half above for its distinct columns, then one Gram kernel sums, for every pair, the products of the two columns'
// lanes over the rows both paths share (the path from their lowest common ancestor to the root) and over the dense top.
// The same runs on right-hand sides given whole, each nonzero on a set of source block columns (covariance_pair_sets_plan,
// covariance_pair_sets_pass): the columns of a BA system over its reduced camera system (schur_covariance.hip).
//
// Right-hand sides given whole (slampp_hip_solve_columns: solve_columns_enqueue below) share the workspace and the dense top's
// tile solves, with unpruned substitutions of their own over the static device plan: a lane per (block row, right-hand side).
//
// Workspace X: n_scalars x k, interleaved -- the k values of a scalar row next to each other (X[row * k + c]): a lane per
// right-hand side then reads and writes a block's rows as whole contiguous lines (d x k doubles), where a column stride of
// n_scalars would make every lane of a wave touch a line of its own.  Rows of the permuted order (Plan::cs_new).  Which
// rows the pruned forward wrote in this pass is told by a stamp per column (d_mark): the backward substitution reads y_j
// only there, zero elsewhere -- no clearing of n_scalars x k doubles per pass.
#include <hip/hip_runtime.h>
#include "covariance.h"
#include "solver.h"
#include "sparse_inverse.h"
#include "pair_plan.h"

#include <algorithm>
#include <climits>

namespace slampp {

struct TCovGather { // 16 B
	int64_t src; // >= 0: offset of the stored block of Z; < 0: -1 - (pos_r << 24 | pos_c), element-wise from the dense top's inverse
	int64_t out; // output offset << 9 | d_r << 5 | d_c << 1 | read transposed
};

struct TCovFwd { // 40 B: one listed column of the pruned forward substitution
	int64_t linv_off; // inv(L_jj)
	int64_t e0;       // first of its filtered row entries
	int32_t ne, dj;
	int32_t ycs;      // scalar offset in the permuted workspace
	int32_t bcol;     // right-hand side c of this pass has its 1 in row c - bcol of this column (if 0 <= c - bcol < dj)
	int32_t dpos;     // dense top: position in the dense system (the column's reduced right-hand side goes there), else -1
	int32_t s;        // schedule index (the stamp goes there)
};

struct TSolveTopCol { // 32 B: one dense-top column of solve_columns_enqueue
	int64_t cs_src;   // scalar offset in the caller's vectors
	int64_t e0;       // first of its row entries L(j,c) with c below the dense top
	int32_t ne, dj;
	int32_t dpos;     // position in the dense system
	int32_t pad;
};

namespace {
struct TCovLaunch {
	int n_stage;       // -1: the dense-top columns
	int seg0, seg1;
};
struct TCovPass {
	int col0, kp;
	std::vector<TCovLaunch> launches;
};
} // anonymous namespace

struct CCovariance {
	// pattern gather
	bool b_gather = false;
	int64_t n_gather = 0;
	int n_gather_dim = 0; // 3 / 6 / 7: every block is D x D; 0: any sizes up to 8
	CDevArray<TCovGather> d_gather;
	// block columns
	bool b_columns = false;
	std::vector<int32_t> sched_pos;   // [n] schedule index of column j (new order), -1 in the dense top
	std::vector<int32_t> sched_task;  // [n_sched] task of a schedule index
	std::vector<int32_t> task_stage;  // [n_tasks]
	std::vector<int32_t> host_mark, host_bcol;
	int32_t n_host_stamp = 0;
	CDevArray<double> d_X, d_Bd, d_Zb;
	CDevArray<int32_t> d_mark;
	int32_t n_stamp = 0;
	// what one call lists: the uploads from these vectors are asynchronous, so a call refills them only once the previous
	// call's uploads have completed (ev_lists, recorded behind them on the handle's stream)
	hipEvent_t ev_lists = 0;
	std::vector<TCovFwd> fwd;
	std::vector<TRowEnt> ents;
	std::vector<int32_t> seg; // segment b: fwd[seg[b] .. seg[b + 1]), the listed columns of one task
	CDevArray<TCovFwd> d_fwd;
	CDevArray<TRowEnt> d_ents;
	CDevArray<int32_t> d_seg;
	std::vector<int32_t> reach, dense_reach; // (List_Pass's scratch)
	// blocks at arbitrary pairs (slampp_hip_marginal_blocks): the records of every pass of one call, uploaded with the lists above
	PairPlan pair_plan;
	std::vector<TPairRec> pairs;
	std::vector<TPairRow> pair_rows;
	CDevArray<TPairRec> d_pairs;
	CDevArray<TPairRow> d_pair_rows;
	std::vector<TCovPass> set_passes; // covariance_pair_sets_plan: the forward substitution of every pass of pair_plan
	// right-hand sides given whole (slampp_hip_solve_columns): the dense-top columns and their row entries L(j,c), c below the
	// top -- a static list, built at the first such call after an analysis
	bool b_solve_top = false;
	int n_top_cols = 0;
	CDevArray<TSolveTopCol> d_top_cols;
	CDevArray<TRowEnt> d_top_ents;
	~CCovariance() { if(ev_lists) (void)hipEventDestroy(ev_lists); }
};

void covariance_destroy(CCovariance *p) { delete p; }

size_t covariance_bytes(const CCovariance *p)
{
	return p? p->d_gather.n_Bytes() + p->d_X.n_Bytes() + p->d_Bd.n_Bytes() + p->d_Zb.n_Bytes() + p->d_mark.n_Bytes() +
		p->d_fwd.n_Bytes() + p->d_ents.n_Bytes() + p->d_seg.n_Bytes() + p->d_pairs.n_Bytes() + p->d_pair_rows.n_Bytes() +
		p->d_top_cols.n_Bytes() + p->d_top_ents.n_Bytes() : 0;
}

// ---- pattern gather ----

__device__ __forceinline__ double cov_gather_value(const TCovGather &g, int a, int b, int dr, int dc, const double *__restrict__ Z,
	const double *__restrict__ Zd, int ld)
{
	if(g.src >= 0)
		return (g.out & 1)? Z[g.src + b + int64_t(a) * dc] : Z[g.src + a + int64_t(b) * dr];
	const int64_t code = -1 - g.src;
	const int64_t pa = (code >> 24) + a, pb = (code & 0xffffff) + b;
	return Zd[((pa > pb)? pa : pb) + ((pa > pb)? pb : pa) * int64_t(ld)];
}

// every block D x D: a thread per output element, the output streamed in order
template <int D>
__global__ void __launch_bounds__(256)
cov_gather_kernel(int64_t n_blocks, const TCovGather *__restrict__ recs, const double *__restrict__ Z, const double *__restrict__ Zd,
	int ld, double *__restrict__ out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(gid >= n_blocks * (D * D))
		return;
	const int64_t blk = gid / (D * D);
	const int e = int(gid - blk * (D * D)), a = e % D, b = e / D;
	const TCovGather g = recs[blk];
	out[gid] = cov_gather_value(g, a, b, D, D, Z, Zd, ld);
}

// any block sizes up to 8: a wave per block
__global__ void __launch_bounds__(256)
cov_gather_any_kernel(int64_t n_blocks, const TCovGather *__restrict__ recs, const double *__restrict__ Z, const double *__restrict__ Zd,
	int ld, double *__restrict__ out)
{
	const int64_t blk = int64_t(blockIdx.x) * (blockDim.x / 64) + threadIdx.x / 64;
	const int e = threadIdx.x & 63;
	if(blk >= n_blocks)
		return;
	const TCovGather g = recs[blk];
	const int dr = int(g.out >> 5) & 15, dc = int(g.out >> 1) & 15;
	if(e < dr * dc)
		out[(g.out >> 9) + e] = cov_gather_value(g, e % dr, e / dr, dr, dc, Z, Zd, ld);
}

static void Setup_Gather(slampp_hip_solver &s, CCovariance &cv)
{
	const Plan &P = s.plan;
	const int64_t n_bcols = int64_t(s.cumsum.size()) - 1;
	const int64_t n_blocks = s.bcol_ptr[size_t(n_bcols)];
	std::vector<TCovGather> recs(static_cast<size_t>(n_blocks));
	bool b_all_same = P.uniform_dim && (P.max_dim == 3 || P.max_dim == 6 || P.max_dim == 7);
	int64_t n_out = 0;
	for(int64_t C = 0; C < n_bcols; ++ C) {
		const int32_t j = P.pinv[size_t(C)];
		const int dc = int(s.cumsum[C + 1] - s.cumsum[C]);
		for(int64_t b = s.bcol_ptr[size_t(C)]; b < s.bcol_ptr[size_t(C + 1)]; ++ b) {
			const int32_t R = s.brow[size_t(b)], i = P.pinv[size_t(R)];
			const int dr = int(s.cumsum[R + 1] - s.cumsum[R]);
			TCovGather &g = recs[size_t(b)];
			int64_t n_trans = 0;
			if(P.dense_dim && P.dense_pos[i] >= 0 && P.dense_pos[j] >= 0)
				g.src = -1 - ((int64_t(P.dense_pos[i]) << 24) | int64_t(P.dense_pos[j]));
			else {
				// Lambda's pattern lies inside the filled pattern of L, whatever the ordering: checked here, once
				g.src = plan_block_offset(P, std::max(i, j), std::min(i, j));
				if(g.src < 0)
					throw std::logic_error("marginals_pattern: a block of Lambda is outside the pattern of its factor");
				n_trans = i < j;
			}
			g.out = (n_out << 9) | (int64_t(dr) << 5) | (int64_t(dc) << 1) | n_trans;
			n_out += int64_t(dr) * dc;
		}
	}
	cv.d_gather.Upload(recs, s.stream);
	SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream)); // recs lives in this scope
	cv.n_gather = n_blocks;
	cv.n_gather_dim = b_all_same? P.max_dim : 0;
	cv.b_gather = true;
}

static CCovariance &Covariance_State(slampp_hip_solver &s)
{
	if(!s.p_cov)
		s.p_cov = new CCovariance();
	return *s.p_cov;
}

void covariance_pattern_enqueue(slampp_hip_solver &s, double *p_out_dev)
{
	CCovariance &cv = Covariance_State(s);
	if(!cv.b_gather)
		Setup_Gather(s, cv);
	if(!cv.n_gather)
		return;
	const double *Z = s.d_Z.p(), *Zd = s.d_Zd.p();
	const int ld = s.n_dense_pad;
	switch(cv.n_gather_dim) {
#define COV_GATHER(DD) case DD: hipLaunchKernelGGL(cov_gather_kernel<DD>, dim3(unsigned((cv.n_gather * (DD * DD) + 255) / 256)), dim3(256), 0, s.stream, \
		cv.n_gather, cv.d_gather.p(), Z, Zd, ld, p_out_dev); break;
	COV_GATHER(3)
	COV_GATHER(6)
	COV_GATHER(7)
#undef COV_GATHER
	default:
		hipLaunchKernelGGL(cov_gather_any_kernel, dim3(unsigned((cv.n_gather + 3) / 4)), dim3(256), 0, s.stream, cv.n_gather,
			cv.d_gather.p(), Z, Zd, ld, p_out_dev);
	}
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- block columns: pruned k-column forward substitution ----

// one workgroup (one wave) per segment: the listed columns of one task, in order; lane c = right-hand side c.  B_RHS: the
// right-hand side is not P E_J but the dense block B (permuted rows, interleaved like X: B[row * kp + c]; nonzero on the
// listed columns' own rows only) -- the landmark columns of the Schur path (schur_covariance.hip)
template <int D, bool B_RHS = false>
__global__ void __launch_bounds__(64)
cov_forward_kernel(const int32_t *__restrict__ seg, int seg_begin, const TCovFwd *__restrict__ fwd, const TRowEnt *__restrict__ ents,
	const double *__restrict__ L, const double *__restrict__ Linv, double *X, int kp, int32_t *mark, int32_t n_stamp,
	double *Bd, const double *__restrict__ B = 0)
{
	constexpr int DM = D? D : 8;
	const int c = threadIdx.x;
	const bool b_act = c < kp;
	const int sg = seg_begin + blockIdx.x;
	for(int32_t f = seg[sg]; f < seg[sg + 1]; ++ f) {
		const TCovFwd rec = fwd[f];
		const int dj = D? D : rec.dj;
		double acc[DM];
		#pragma unroll
		for(int r = 0; r < DM; ++ r) {
			if(B_RHS)
				acc[r] = (r < dj && b_act)? B[int64_t(rec.ycs + r) * kp + c] : 0.0;
			else
				acc[r] = (c - rec.bcol == r)? 1.0 : 0.0; // the right-hand side's block: P E_J
		}
		for(int64_t e = rec.e0; e < rec.e0 + rec.ne; ++ e) {
			const TRowEnt t_e = ents[e];
			const int dc = D? D : t_e.dc;
			const double *Lb = L + t_e.off; // L(j,c): dj x dc
			#pragma unroll
			for(int t = 0; t < DM; ++ t) {
				if(t < dc) {
					const double yv = b_act? X[int64_t(t_e.ycs + t) * kp + c] : 0.0;
					#pragma unroll
					for(int r = 0; r < DM; ++ r) {
						if(r < dj)
							acc[r] -= Lb[r + t * dj] * yv;
					}
				}
			}
		}
		if(rec.dpos >= 0) { // a dense-top column: its reduced right-hand side, for the dense solve
			#pragma unroll
			for(int r = 0; r < DM; ++ r) {
				if(r < dj && b_act)
					Bd[int64_t(rec.dpos + r) * kp + c] = acc[r];
			}
			continue;
		}
		const double *iL = Linv + rec.linv_off;
		#pragma unroll
		for(int r = 0; r < DM; ++ r) {
			if(r < dj) {
				double y = 0;
				#pragma unroll
				for(int t = 0; t < DM; ++ t) {
					if(t < dj)
						y += iL[r + t * dj] * acc[t];
				}
				if(b_act)
					X[int64_t(rec.ycs + r) * kp + c] = y; // (read later by this very lane only: no barrier)
			}
		}
		if(c == 0)
			mark[rec.s] = n_stamp;
	}
}

// ---- block columns: k-column backward substitution over all stages ----

// one wave per task, its columns last to first (as backward_stage_kernel); x_j = inv(L_jj)^T (y_j - sum L(i,j)^T x_i)
template <int D>
__global__ void __launch_bounds__(64)
cov_backward_kernel(const TColDesc *__restrict__ cols, const TBlkDesc *__restrict__ blks, const int64_t *__restrict__ task_ptr,
	int task_begin, const double *__restrict__ L, const double *__restrict__ Linv, double *X, int kp,
	const int32_t *__restrict__ mark, int32_t n_stamp, double *__restrict__ out, int64_t n_scalars, int col0)
{
	constexpr int DM = D? D : 8;
	const int c = threadIdx.x;
	const bool b_act = c < kp;
	const int task = task_begin + blockIdx.x;
	for(int64_t sc = task_ptr[task + 1] - 1; sc >= task_ptr[task]; -- sc) {
		const TColDesc cd = cols[sc];
		const int dj = D? D : cd.dj;
		const bool b_y = mark[sc] == n_stamp; // the pruned forward substitution wrote y_j in this pass
		double acc[DM];
		#pragma unroll
		for(int r = 0; r < DM; ++ r)
			acc[r] = (r < dj && b_y && b_act)? X[(cd.cs_new + r) * kp + c] : 0.0;
		for(int64_t b = cd.k0 + 1; b < cd.k0 + cd.nb; ++ b) {
			const TBlkDesc bd = blks[b];
			const int di = D? D : int(bd.np_di >> 24);
			const double *Lb = L + bd.loff; // L(i,j): di x dj
			#pragma unroll
			for(int t = 0; t < DM; ++ t) {
				if(t < di) {
					const double xv = b_act? X[int64_t(bd.xcs + t) * kp + c] : 0.0;
					#pragma unroll
					for(int r = 0; r < DM; ++ r) {
						if(r < dj)
							acc[r] -= Lb[t + r * di] * xv;
					}
				}
			}
		}
		const double *iL = Linv + cd.linv_off;
		#pragma unroll
		for(int r = 0; r < DM; ++ r) {
			if(r < dj) {
				double x = 0;
				#pragma unroll
				for(int t = 0; t < DM; ++ t) {
					if(t < dj)
						x += iL[t + r * dj] * acc[t];
				}
				if(b_act) {
					X[(cd.cs_new + r) * kp + c] = x;
					out[cd.cs_src + r + (int64_t(col0) + c) * n_scalars] = x;
				}
			}
		}
	}
}

// ---- block columns: the dense top, k columns, tile by tile ----

enum { COV_NB = 64 };

// forward step of tile column t: every workgroup forms z_t = inv(L_tt) b_t itself; workgroup 0 publishes it, workgroup
// g > 0 subtracts L(t + g, t) z_t from b_{t + g}.  Positions >= n (padding, the right-hand side row of the factor) are zero.
__global__ void __launch_bounds__(256)
cov_dense_forward_kernel(const double *__restrict__ M, int ld, int n, int t, const double *__restrict__ invdiag, double *Bd,
	double *Zb, int kp)
{
	__shared__ double s_b[COV_NB * COV_K_PASS], s_z[COV_NB * COV_K_PASS];
	const int ne = COV_NB * kp, t0 = t * COV_NB;
	for(int e = threadIdx.x; e < ne; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		s_b[e] = (t0 + i < n)? Bd[int64_t(t0 + i) * kp + c] : 0.0;
	}
	__syncthreads();
	const double *iL = invdiag + size_t(t) * COV_NB * COV_NB;
	for(int e = threadIdx.x; e < ne; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		double z = 0;
		if(t0 + i < n) {
			for(int q = 0; q <= i; ++ q)
				z += iL[i + q * COV_NB] * s_b[q * kp + c];
		}
		s_z[e] = z;
	}
	__syncthreads();
	if(blockIdx.x == 0) {
		for(int e = threadIdx.x; e < ne; e += blockDim.x) {
			const int i = e / kp, c = e - i * kp;
			Zb[int64_t(t0 + i) * kp + c] = s_z[e];
		}
		return;
	}
	const int g0 = (t + int(blockIdx.x)) * COV_NB;
	const int n_q = (n - t0 < COV_NB)? n - t0 : int(COV_NB);
	for(int e = threadIdx.x; e < ne; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		if(g0 + i >= n)
			continue;
		const double *Mr = M + (g0 + i) + size_t(t0) * ld;
		double acc = 0;
		for(int q = 0; q < n_q; ++ q)
			acc += Mr[size_t(q) * ld] * s_z[q * kp + c];
		Bd[int64_t(g0 + i) * kp + c] -= acc;
	}
}

// backward step of tile column t: every workgroup forms x_t = inv(L_tt)^T z_t itself; workgroup t stores it (into X at the
// column's permuted rows, and into the output at the caller's), workgroup g < t subtracts L(t, g)^T x_t from z_g
__global__ void __launch_bounds__(256)
cov_dense_backward_kernel(const double *__restrict__ M, int ld, int n, int t, const double *__restrict__ invdiag, double *Zb, int kp,
	const longlong2 *__restrict__ dst, double *X, double *out, int64_t n_scalars, int col0)
{
	__shared__ double s_z[COV_NB * COV_K_PASS], s_x[COV_NB * COV_K_PASS];
	const int ne = COV_NB * kp, t0 = t * COV_NB;
	const int n_q = (n - t0 < COV_NB)? n - t0 : int(COV_NB);
	for(int e = threadIdx.x; e < ne; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		s_z[e] = (t0 + i < n)? Zb[int64_t(t0 + i) * kp + c] : 0.0;
	}
	__syncthreads();
	const double *iL = invdiag + size_t(t) * COV_NB * COV_NB;
	for(int e = threadIdx.x; e < ne; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		double x = 0;
		for(int q = i; q < n_q; ++ q)
			x += iL[q + i * COV_NB] * s_z[q * kp + c];
		s_x[e] = x;
	}
	__syncthreads();
	if(int(blockIdx.x) == t) {
		for(int e = threadIdx.x; e < ne; e += blockDim.x) {
			const int i = e / kp, c = e - i * kp;
			if(t0 + i >= n)
				continue;
			const longlong2 d = dst[t0 + i];
			if(d.x >= 0) {
				X[d.x * kp + c] = s_x[e];
				out[d.y + (int64_t(col0) + c) * n_scalars] = s_x[e];
			}
		}
		return;
	}
	const int g0 = int(blockIdx.x) * COV_NB;
	for(int e = threadIdx.x; e < ne; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		if(g0 + i >= n)
			continue;
		const double *Mc = M + t0 + size_t(g0 + i) * ld; // column g0 + i of L, rows t0 ..
		double acc = 0;
		for(int q = 0; q < n_q; ++ q)
			acc += Mc[q] * s_x[q * kp + c];
		Zb[int64_t(g0 + i) * kp + c] -= acc;
	}
}

static void Setup_Columns(slampp_hip_solver &s, CCovariance &cv)
{
	const Plan &P = s.plan;
	const int64_t n_sched = int64_t(P.task_cols.size());
	const int n_tasks = int(P.task_ptr.size()) - 1, n_stages = int(P.stage_ptr.size()) - 1;
	cv.sched_pos.assign(size_t(P.n), -1);
	cv.sched_task.assign(size_t(n_sched), 0);
	cv.task_stage.assign(size_t(std::max(n_tasks, 0)), 0);
	for(int64_t sc = 0; sc < n_sched; ++ sc)
		cv.sched_pos[size_t(P.task_cols[size_t(sc)])] = int32_t(sc);
	for(int t = 0; t < n_tasks; ++ t) {
		for(int64_t sc = P.task_ptr[size_t(t)]; sc < P.task_ptr[size_t(t + 1)]; ++ sc)
			cv.sched_task[size_t(sc)] = t;
	}
	for(int st = 0; st < n_stages; ++ st) {
		for(int t = P.stage_ptr[size_t(st)]; t < P.stage_ptr[size_t(st + 1)]; ++ t)
			cv.task_stage[size_t(t)] = st;
	}
	cv.host_mark.assign(size_t(P.n), 0);
	cv.host_bcol.assign(size_t(P.n), INT_MIN / 2);
	cv.n_host_stamp = 0;
	cv.d_X.Alloc(size_t(s.n_scalars) * COV_K_PASS);
	cv.d_mark.Alloc(size_t(std::max<int64_t>(n_sched, 1)));
	SLAMPP_HIP_CHECK(hipMemsetAsync(cv.d_mark.p(), 0, cv.d_mark.n_Bytes(), s.stream));
	cv.n_stamp = 0;
	if(s.n_dense_dim) {
		cv.d_Bd.Alloc(size_t(s.n_dense_pad) * COV_K_PASS);
		cv.d_Zb.Alloc(size_t(s.n_dense_pad) * COV_K_PASS);
	}
	cv.b_columns = true;
}

// The lists of one call are built before anything is enqueued and go up in one set of uploads: Lists_Begin(), List_Pass()
// per pass, Lists_Upload().
static void Lists_Begin(CCovariance &cv)
{
	if(cv.ev_lists)
		SLAMPP_HIP_CHECK(hipEventSynchronize(cv.ev_lists)); // (the previous call's uploads out of these vectors are over)
	cv.fwd.clear();
	cv.ents.clear();
	cv.seg.assign(1, 0);
	cv.pairs.clear();
	cv.pair_rows.clear();
}

// lists the pruned forward substitution of one pass: the union of the paths of the columns p_src[0 .. n_src) (new order) to
// the root, stage by stage.  p_lane[i]: where the unit right-hand sides of column p_src[i] start among the pass's lanes
// (negative where the column begins in the pass before); p_lane = 0: the right-hand sides are given whole
static void List_Pass(CCovariance &cv, const Plan &P, int n_src, const int32_t *p_src, const int32_t *p_lane, TCovPass &pass)
{
	if(++ cv.n_host_stamp == INT_MAX) {
		std::fill(cv.host_mark.begin(), cv.host_mark.end(), 0);
		cv.n_host_stamp = 1;
	}
	const int32_t n_hs = cv.n_host_stamp;
	std::vector<int32_t> &reach = cv.reach, &dense_reach = cv.dense_reach;
	reach.clear();
	dense_reach.clear();
	for(int i = 0; i < n_src; ++ i) {
		const int32_t j = p_src[i];
		if(p_lane)
			cv.host_bcol[size_t(j)] = p_lane[i];
		for(int32_t x = j; x >= 0 && cv.host_mark[size_t(x)] != n_hs; x = P.parent[size_t(x)]) {
			cv.host_mark[size_t(x)] = n_hs;
			if(cv.sched_pos[size_t(x)] >= 0)
				reach.push_back(x);
			else
				dense_reach.push_back(x);
		}
	}
	std::sort(reach.begin(), reach.end(), [&](int32_t a, int32_t b) { return cv.sched_pos[size_t(a)] < cv.sched_pos[size_t(b)]; });
	std::sort(dense_reach.begin(), dense_reach.end());
	int n_cur_task = -1, n_cur_stage = -1;
	for(int h = 0; h < 2; ++ h) { // the block-eliminated columns stage by stage, then the dense-top ones
		const std::vector<int32_t> &r_list = h? dense_reach : reach;
		for(size_t q = 0; q < r_list.size(); ++ q) {
			const int32_t j = r_list[q];
			const int32_t sc = cv.sched_pos[size_t(j)];
			const int n_task = h? -2 - int(q) : cv.sched_task[size_t(sc)];
			const int n_stage = h? -1 : cv.task_stage[size_t(n_task)];
			if(n_task != n_cur_task) { // a segment of its own
				if(n_cur_task != -1)
					cv.seg.push_back(int32_t(cv.fwd.size()));
				if(n_stage != n_cur_stage || pass.launches.empty()) {
					TCovLaunch l = {n_stage, int(cv.seg.size()) - 1, int(cv.seg.size()) - 1};
					pass.launches.push_back(l);
				}
				pass.launches.back().seg1 ++;
				n_cur_task = n_task;
				n_cur_stage = n_stage;
			}
			TCovFwd f;
			f.linv_off = (sc >= 0)? P.linv_off[size_t(j)] : 0;
			f.e0 = int64_t(cv.ents.size());
			f.dj = P.dim[size_t(j)];
			f.ycs = int32_t(P.cs_new[size_t(j)]);
			f.bcol = cv.host_bcol[size_t(j)];
			f.dpos = (sc >= 0)? -1 : P.dense_pos[size_t(j)];
			f.s = std::max(sc, 0);
			for(int64_t r = P.rptr[size_t(j)]; r < P.rptr[size_t(j) + 1]; ++ r) {
				const int32_t b = P.rblk[size_t(r)], c = P.blk_col[size_t(b)];
				if(cv.host_mark[size_t(c)] != n_hs || cv.sched_pos[size_t(c)] < 0)
					continue; // y_c is zero in this pass, or c is in the dense top (its part is the dense solve's)
				TRowEnt t_e;
				t_e.off = P.loff[size_t(b)];
				t_e.ycs = int32_t(P.cs_new[size_t(c)]);
				t_e.dc = P.dim[size_t(c)];
				cv.ents.push_back(t_e);
			}
			f.ne = int32_t(int64_t(cv.ents.size()) - f.e0);
			cv.fwd.push_back(f);
		}
	}
	if(n_cur_task != -1)
		cv.seg.push_back(int32_t(cv.fwd.size()));
	for(int i = 0; i < n_src; ++ i)
		cv.host_bcol[size_t(p_src[i])] = INT_MIN / 2;
}

static void Lists_Upload(slampp_hip_solver &s, CCovariance &cv)
{
	if(cv.fwd.empty())
		cv.fwd.resize(1); // (nothing listed: a record nobody reads, so that the uploads below have something to send)
	if(cv.ents.empty())
		cv.ents.resize(1);
	cv.d_fwd.Upload(cv.fwd, s.stream);
	cv.d_ents.Upload(cv.ents, s.stream);
	cv.d_seg.Upload(cv.seg, s.stream);
	if(!cv.pairs.empty()) { // (slampp_hip_marginal_blocks)
		if(cv.pair_rows.empty())
			cv.pair_rows.resize(1);
		cv.d_pairs.Upload(cv.pairs, s.stream);
		cv.d_pair_rows.Upload(cv.pair_rows, s.stream);
	}
	if(!cv.ev_lists)
		SLAMPP_HIP_CHECK(hipEventCreateWithFlags(&cv.ev_lists, hipEventDisableTiming));
	SLAMPP_HIP_CHECK(hipEventRecord(cv.ev_lists, s.stream));
}

static int Unrolled_Dim(const Plan &P)
{
	return (P.uniform_dim && (P.max_dim == 3 || P.max_dim == 6 || P.max_dim == 7))? P.max_dim : 0;
}

// the forward half of one pass: a new stamp, the pruned forward substitution into d_X (and the dense-top columns' reduced
// right-hand sides into d_Bd), then -- b_dense_top -- the dense tiles' forward substitution into d_Zb
static void Forward_Enqueue(slampp_hip_solver &s, CCovariance &cv, const TCovPass &pass, const double *p_rhs, bool b_dense_top)
{
	const int D = Unrolled_Dim(s.plan);
	const int ld = s.n_dense_pad, n_dense = s.n_dense_dim, n_tiles = ld / COV_NB;
	const int kp = pass.kp;
	if(++ cv.n_stamp == INT_MAX) {
		SLAMPP_HIP_CHECK(hipMemsetAsync(cv.d_mark.p(), 0, cv.d_mark.n_Bytes(), s.stream));
		cv.n_stamp = 1;
	}
	if(n_dense)
		SLAMPP_HIP_CHECK(hipMemsetAsync(cv.d_Bd.p(), 0, size_t(ld) * kp * sizeof(double), s.stream));
	for(size_t q = 0; q < pass.launches.size(); ++ q) {
		const TCovLaunch &l = pass.launches[q];
		const int n_blocks = l.seg1 - l.seg0;
		const int DL = (l.n_stage < 0)? 0 : D; // (the dense-top columns' dimensions: any)
#define COV_FWD(DD, BR) hipLaunchKernelGGL((cov_forward_kernel<DD, BR>), dim3(n_blocks), dim3(64), 0, s.stream, cv.d_seg.p(), l.seg0, \
			cv.d_fwd.p(), cv.d_ents.p(), s.d_L.p(), s.d_Linv.p(), cv.d_X.p(), kp, cv.d_mark.p(), cv.n_stamp, cv.d_Bd.p(), p_rhs)
		if(p_rhs) {
			switch(DL) {
			case 3: COV_FWD(3, true); break;
			case 6: COV_FWD(6, true); break;
			case 7: COV_FWD(7, true); break;
			default: COV_FWD(0, true); break;
			}
		} else {
			switch(DL) {
			case 3: COV_FWD(3, false); break;
			case 6: COV_FWD(6, false); break;
			case 7: COV_FWD(7, false); break;
			default: COV_FWD(0, false); break;
			}
		}
#undef COV_FWD
	}
	if(n_dense && b_dense_top) {
		for(int t = 0; t < n_tiles; ++ t)
			hipLaunchKernelGGL(cov_dense_forward_kernel, dim3(n_tiles - t), dim3(256), 0, s.stream, s.d_dense.p(), ld, n_dense, t,
				s.d_dense_invdiag.p(), cv.d_Bd.p(), cv.d_Zb.p(), kp);
	}
}

// the backward half: the dense tiles' backward substitution, then every stage's, last to first; x goes to
// p_out_dev + n_col0 * n_ld_out as each column is finished
static void Backward_Enqueue(slampp_hip_solver &s, CCovariance &cv, const TCovPass &pass, double *p_out_dev, int64_t n_ld_out,
	int64_t n_col0)
{
	const Plan &P = s.plan;
	const int D = Unrolled_Dim(P);
	const int n_stages = int(P.stage_ptr.size()) - 1;
	const int ld = s.n_dense_pad, n_dense = s.n_dense_dim, n_tiles = ld / COV_NB;
	const int kp = pass.kp;
	if(n_dense) {
		for(int t = n_tiles - 1; t >= 0; -- t)
			hipLaunchKernelGGL(cov_dense_backward_kernel, dim3(t + 1), dim3(256), 0, s.stream, s.d_dense.p(), ld, n_dense, t,
				s.d_dense_invdiag.p(), cv.d_Zb.p(), kp, s.d_dense_dst.p(), cv.d_X.p(), p_out_dev, n_ld_out, int(n_col0 + pass.col0));
	}
	for(int st = n_stages - 1; st >= 0; -- st) {
		const int n_tasks = P.stage_ptr[size_t(st + 1)] - P.stage_ptr[size_t(st)];
		if(n_tasks <= 0)
			continue;
#define COV_BWD(DD) hipLaunchKernelGGL(cov_backward_kernel<DD>, dim3(n_tasks), dim3(64), 0, s.stream, s.dplan.cols, s.dplan.blks, \
			s.dplan.task_ptr, P.stage_ptr[size_t(st)], s.d_L.p(), s.d_Linv.p(), cv.d_X.p(), kp, cv.d_mark.p(), cv.n_stamp, p_out_dev, \
			n_ld_out, int(n_col0 + pass.col0))
		switch(D) {
		case 3: COV_BWD(3); break;
		case 6: COV_BWD(6); break;
		case 7: COV_BWD(7); break;
		default: COV_BWD(0); break;
		}
#undef COV_BWD
	}
}

// p_rhs = 0: the unit right-hand sides of the block columns p_bcols, in passes of COV_K_PASS; else one pass of n_rhs_k
// right-hand sides read from p_rhs (see cov_forward_kernel), nonzero on the rows of the block columns p_bcols only.  The
// result goes to p_out_dev + n_col0 * n_ld_out, column-major with leading dimension n_ld_out.
static void columns_enqueue(slampp_hip_solver &s, int n_cols, const int64_t *p_bcols, const double *p_rhs, int n_rhs_k,
	double *p_out_dev, int64_t n_ld_out, int64_t n_col0)
{
	const Plan &P = s.plan;
	CCovariance &cv = Covariance_State(s);
	if(!cv.b_columns)
		Setup_Columns(s, cv);
	int64_t k = 0;
	std::vector<int64_t> col_off(size_t(n_cols) + 1, 0);
	for(int i = 0; i < n_cols; ++ i) {
		col_off[size_t(i)] = (p_rhs)? 0 : k; // (one pass over all the sources)
		k += s.cumsum[size_t(p_bcols[i] + 1)] - s.cumsum[size_t(p_bcols[i])];
	}
	if(p_rhs) {
		if(n_rhs_k <= 0 || n_rhs_k > COV_K_PASS)
			throw std::invalid_argument("marginal_columns: a right-hand side block of 1 .. COV_K_PASS columns");
		k = n_rhs_k;
		std::fill(col_off.begin(), col_off.end(), int64_t(0));
		col_off[size_t(n_cols)] = k;
	}
	col_off[size_t(n_cols)] = k;
	if(k > int64_t(INT_MAX))
		throw std::invalid_argument("marginal_columns: too many columns");
	Lists_Begin(cv);
	std::vector<TCovPass> passes;
	std::vector<int32_t> src, lane;
	for(int64_t col0 = 0; col0 < k; col0 += COV_K_PASS) {
		TCovPass pass;
		pass.col0 = int(col0);
		pass.kp = int(std::min<int64_t>(COV_K_PASS, k - col0));
		src.clear();
		lane.clear();
		for(int i = 0; i < n_cols; ++ i) {
			if(!p_rhs && (col_off[size_t(i) + 1] <= col0 || col_off[size_t(i)] >= col0 + pass.kp))
				continue; // not in this pass
			src.push_back(P.pinv[size_t(p_bcols[i])]);
			lane.push_back(int32_t(col_off[size_t(i)] - col0));
		}
		List_Pass(cv, P, int(src.size()), src.data(), p_rhs? 0 : lane.data(), pass);
		passes.push_back(pass);
	}
	Lists_Upload(s, cv);
	s.Phase_Begin("marginal_columns");
	for(size_t p = 0; p < passes.size(); ++ p) {
		Forward_Enqueue(s, cv, passes[p], p_rhs, true);
		Backward_Enqueue(s, cv, passes[p], p_out_dev, n_ld_out, n_col0);
	}
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- right-hand sides given whole (slampp_hip_solve_columns): both substitutions over the static plan ----
//
// Nothing is pruned and nothing is listed per call: the kernels walk TDevPlan::cols / rents / blks / task_ptr, the records of
// the single-vector substitutions, one launch per stage.  A lane owns one (row r of the block, right-hand side c) pair: with
// blocks of dimension D a wave carries 64 / D right-hand sides (21 at D = 3, 10 at D = 6, 9 at D = 7; 8 with mixed
// dimensions, each right-hand side eight lanes apart), further right-hand sides of the same task go to further workgroups
// (blockIdx.y).  A lane sums its row of every block product in the order of the records, so what column c gets depends on
// column c alone -- not on k, not on where c sits in a wave -- and never meets another column's numbers (a NaN stays in its
// column).  The product with inv(L_jj) needs the other rows of the same c: they come from the neighbouring lanes by
// __shfl.  The forward kernel reads column c of the caller's array at TColDesc::cs_src (the permutation is fused in) and
// writes the interleaved workspace X[row * kp + c]; the backward kernel writes X and the caller's array.

template <int D>
struct TSolveLanes {
	enum { DM = D? D : 8, PER_WAVE = 64 / DM };
	int r, c, base; // row of the block, right-hand side of the pass, lane of row 0 of that right-hand side
	bool b_rhs;     // the lane has a right-hand side at all
	__device__ __forceinline__ TSolveLanes(int kp)
	{
		const int lane = threadIdx.x, cl = lane / DM;
		r = lane - cl * DM;
		base = cl * DM;
		c = int(blockIdx.y) * PER_WAVE + cl;
		b_rhs = cl < PER_WAVE && c < kp;
		if(!b_rhs)
			c = 0; // (addresses stay valid; nothing of such a lane is stored)
	}
};

// records a lane has in flight at a time: the loads of a batch -- the records, then every block element and vector entry they
// name -- are issued together, so a batch costs two trips to memory where record by record every record costs two.  The sum
// itself goes on in the order of the records (a record past the end adds products of zeros, which change nothing)
template <int D>
struct TSolveBatch {
	enum { N = D? 4 : 2 };
};

// acc - sum over the row entries e0 .. e0 + ne of row r of L(j,c') y_c'
template <int D>
__device__ __forceinline__ double solve_cols_row_sum(double acc, const TRowEnt *__restrict__ ents, int64_t e0, int ne, int dj,
	const double *__restrict__ L, const double *X, int kp, int r, int c, bool b_act)
{
	constexpr int DM = D? D : 8, NB = TSolveBatch<D>::N;
	const int64_t e_end = e0 + ne;
	for(int64_t e = e0; e < e_end; e += NB) {
		double lv[NB][DM], xv[NB][DM];
		#pragma unroll
		for(int u = 0; u < NB; ++ u) {
			const bool b_on = b_act && e + u < e_end;
			const TRowEnt t_e = ents[(e + u < e_end)? e + u : e]; // (a record of this column either way)
			const int dc = D? D : t_e.dc;
			const double *Lb = L + t_e.off + r; // L(j,c'): dj x dc
			const double *Xc = X + int64_t(t_e.ycs) * kp + c;
			#pragma unroll
			for(int t = 0; t < DM; ++ t) {
				lv[u][t] = (b_on && t < dc)? Lb[t * dj] : 0.0;
				xv[u][t] = (b_on && t < dc)? Xc[int64_t(t) * kp] : 0.0;
			}
		}
		#pragma unroll
		for(int u = 0; u < NB; ++ u) {
			#pragma unroll
			for(int t = 0; t < DM; ++ t)
				acc -= lv[u][t] * xv[u][t];
		}
	}
	return acc;
}

// forward substitution of one stage: a workgroup (one wave) per task and group of right-hand sides, the task's columns in order
template <int D>
__global__ void __launch_bounds__(64)
solve_cols_forward_kernel(const TColDesc *__restrict__ cols, const TRowEnt *__restrict__ rents, const int64_t *__restrict__ task_ptr,
	int task_begin, const double *__restrict__ L, const double *__restrict__ Linv, const double *rhs, int64_t n_ld, double *X, int kp)
{
	constexpr int DM = D? D : 8;
	const TSolveLanes<D> m(kp);
	const int task = task_begin + blockIdx.x;
	const int64_t sc_end = task_ptr[task + 1];
	for(int64_t sc = task_ptr[task]; sc < sc_end; ++ sc) {
		const TColDesc cd = cols[sc];
		const int dj = D? D : cd.dj;
		const bool b_act = m.b_rhs && m.r < dj;
		const int r = b_act? m.r : 0;
		double acc = b_act? rhs[cd.cs_src + r + int64_t(m.c) * n_ld] : 0.0;
		acc = solve_cols_row_sum<D>(acc, rents, cd.r0, cd.nr, dj, L, X, kp, r, m.c, b_act);
		const double *iL = Linv + cd.linv_off;
		double y = 0;
		#pragma unroll
		for(int t = 0; t < DM; ++ t) {
			if(t < dj) {
				const double vt = __shfl(acc, m.base + t); // (every lane of the wave takes part)
				if(t <= r)
					y += iL[r + t * dj] * vt;
			}
		}
		if(b_act)
			X[(cd.cs_new + r) * kp + m.c] = y;
		__syncthreads(); // single-wave workgroup: y_j is where the following columns' other rows look for it
	}
}

// the reduced right-hand sides of the dense-top columns, for the dense tiles' substitutions: a workgroup per column and group
template <int D>
__global__ void __launch_bounds__(64)
solve_cols_top_kernel(const TSolveTopCol *__restrict__ top, const TRowEnt *__restrict__ ents, const double *__restrict__ L,
	const double *rhs, int64_t n_ld, const double *X, int kp, double *Bd)
{
	const TSolveLanes<D> m(kp);
	const TSolveTopCol rec = top[blockIdx.x];
	const int dj = D? D : rec.dj;
	const bool b_act = m.b_rhs && m.r < dj;
	const int r = b_act? m.r : 0;
	double acc = b_act? rhs[rec.cs_src + r + int64_t(m.c) * n_ld] : 0.0;
	acc = solve_cols_row_sum<D>(acc, ents, rec.e0, rec.ne, dj, L, X, kp, r, m.c, b_act);
	if(b_act)
		Bd[int64_t(rec.dpos + r) * kp + m.c] = acc;
}

// backward substitution of one stage, the task's columns last to first: x_j = inv(L_jj)^T (y_j - sum L(i,j)^T x_i); lane
// (r, c) sums column r of every block L(i,j) against x_i of right-hand side c
template <int D>
__global__ void __launch_bounds__(64)
solve_cols_backward_kernel(const TColDesc *__restrict__ cols, const TBlkDesc *__restrict__ blks, const int64_t *__restrict__ task_ptr,
	int task_begin, const double *__restrict__ L, const double *__restrict__ Linv, double *X, int kp, double *out, int64_t n_ld)
{
	constexpr int DM = D? D : 8, NB = TSolveBatch<D>::N;
	const TSolveLanes<D> m(kp);
	const int task = task_begin + blockIdx.x;
	const int64_t sc_begin = task_ptr[task];
	for(int64_t sc = task_ptr[task + 1] - 1; sc >= sc_begin; -- sc) {
		const TColDesc cd = cols[sc];
		const int dj = D? D : cd.dj;
		const bool b_act = m.b_rhs && m.r < dj;
		const int r = b_act? m.r : 0;
		double acc = b_act? X[(cd.cs_new + r) * kp + m.c] : 0.0;
		const int64_t b_end = cd.k0 + cd.nb;
		for(int64_t b = cd.k0 + 1; b < b_end; b += NB) { // (in batches, as solve_cols_row_sum)
			double lv[NB][DM], xv[NB][DM];
			#pragma unroll
			for(int u = 0; u < NB; ++ u) {
				const bool b_on = b_act && b + u < b_end;
				const TBlkDesc &bd = blks[(b + u < b_end)? b + u : b];
				const int di = D? D : int(bd.np_di >> 24);
				const double *Lb = L + bd.loff + r * di; // L(i,j): di x dj, its column r
				const double *Xi = X + int64_t(bd.xcs) * kp + m.c;
				#pragma unroll
				for(int t = 0; t < DM; ++ t) {
					lv[u][t] = (b_on && t < di)? Lb[t] : 0.0;
					xv[u][t] = (b_on && t < di)? Xi[int64_t(t) * kp] : 0.0;
				}
			}
			#pragma unroll
			for(int u = 0; u < NB; ++ u) {
				#pragma unroll
				for(int t = 0; t < DM; ++ t)
					acc -= lv[u][t] * xv[u][t];
			}
		}
		const double *iL = Linv + cd.linv_off;
		double x = 0;
		#pragma unroll
		for(int t = 0; t < DM; ++ t) {
			if(t < dj) {
				const double vt = __shfl(acc, m.base + t);
				if(t >= r)
					x += iL[t + r * dj] * vt;
			}
		}
		if(b_act) {
			X[(cd.cs_new + r) * kp + m.c] = x; // (y_j was read by this very lane)
			out[cd.cs_src + r + int64_t(m.c) * n_ld] = x;
		}
		__syncthreads(); // x_j is where the columns before it look for it
	}
}

// the dense-top columns and their row entries below the top (once per analysis)
static void Setup_Solve_Top(slampp_hip_solver &s, CCovariance &cv)
{
	const Plan &P = s.plan;
	std::vector<TSolveTopCol> top;
	std::vector<TRowEnt> ents;
	for(int32_t j = 0; s.n_dense_dim && j < P.n; ++ j) {
		if(cv.sched_pos[size_t(j)] >= 0)
			continue; // (a block-eliminated column)
		TSolveTopCol rec;
		rec.cs_src = P.cs_src[size_t(j)];
		rec.e0 = int64_t(ents.size());
		rec.dj = P.dim[size_t(j)];
		rec.dpos = P.dense_pos[size_t(j)];
		rec.pad = 0;
		for(int64_t r = P.rptr[size_t(j)]; r < P.rptr[size_t(j) + 1]; ++ r) {
			const int32_t b = P.rblk[size_t(r)], c = P.blk_col[size_t(b)];
			if(cv.sched_pos[size_t(c)] < 0)
				continue; // (c is in the dense top: its part is the dense solve's)
			TRowEnt t_e;
			t_e.off = P.loff[size_t(b)];
			t_e.ycs = int32_t(P.cs_new[size_t(c)]);
			t_e.dc = P.dim[size_t(c)];
			ents.push_back(t_e);
		}
		rec.ne = int32_t(int64_t(ents.size()) - rec.e0);
		top.push_back(rec);
	}
	cv.n_top_cols = int(top.size());
	cv.d_top_cols.Upload(top, s.stream);
	cv.d_top_ents.Upload(ents, s.stream);
	SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream)); // the host vectors live in this scope
	cv.b_solve_top = true;
}

bool solve_columns_applies(const slampp_hip_solver &s)
{
	return !s.b_refined && s.plan.max_dim <= 8;
}

// ---- the way in and out between the two substitutions (slampp_hip_solve_half_columns) ----
//
// Transposes between the interleaved workspace (row * kp + c) and the caller's columns (c * n_ld + row), HALF_TILE_ROWS rows
// to a workgroup through an LDS tile, so that both sides move whole lines: the interleaved side as one contiguous run of
// HALF_TILE_ROWS * kp doubles, the caller's side as HALF_TILE_ROWS consecutive doubles of every column.  A tile row is kp | 1
// doubles long: the side that walks down a tile column then has an odd stride in doubles, which puts the 32 lanes of a
// ds_read_b64 group (and the 16 of a write's 128 bytes per clock) on banks of their own.  p_map = 0: interleaved row i is the
// caller's row i (the workspace X).  Otherwise the interleaved rows are the dense top's positions (Zb) and p_map[i].x the
// permuted row of position i, negative for padding and gaps: those are skipped on the way out and zero on the way in.

enum { HALF_TILE_ROWS = 64, HALF_TILE_LD = COV_K_PASS | 1 };

// factor order out: p_cols[c * n_ld + row] = p_inter[i * kp + c]
__global__ void __launch_bounds__(256)
half_export_kernel(const double *__restrict__ p_inter, int64_t n_rows, int kp, const longlong2 *__restrict__ p_map,
	double *__restrict__ p_cols, int64_t n_ld)
{
	__shared__ double s_tile[HALF_TILE_ROWS * HALF_TILE_LD];
	const int64_t r0 = int64_t(blockIdx.x) * HALF_TILE_ROWS;
	const int n_here = int((n_rows - r0 < HALF_TILE_ROWS)? n_rows - r0 : int64_t(HALF_TILE_ROWS));
	for(int e = threadIdx.x; e < n_here * kp; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		s_tile[i * HALF_TILE_LD + c] = p_inter[r0 * kp + e];
	}
	__syncthreads();
	for(int e = threadIdx.x; e < kp * HALF_TILE_ROWS; e += blockDim.x) {
		const int c = e / HALF_TILE_ROWS, i = e - c * HALF_TILE_ROWS;
		if(i >= n_here)
			continue;
		const int64_t row = p_map? int64_t(p_map[r0 + i].x) : r0 + i;
		if(row >= 0)
			p_cols[int64_t(c) * n_ld + row] = s_tile[i * HALF_TILE_LD + c];
	}
}

// factor order in: p_inter[i * kp + c] = p_cols[c * n_ld + row], zero where the position has no row
__global__ void __launch_bounds__(256)
half_import_kernel(const double *__restrict__ p_cols, int64_t n_ld, int64_t n_rows, int kp, const longlong2 *__restrict__ p_map,
	double *__restrict__ p_inter)
{
	__shared__ double s_tile[HALF_TILE_ROWS * HALF_TILE_LD];
	const int64_t r0 = int64_t(blockIdx.x) * HALF_TILE_ROWS;
	const int n_here = int((n_rows - r0 < HALF_TILE_ROWS)? n_rows - r0 : int64_t(HALF_TILE_ROWS));
	for(int e = threadIdx.x; e < kp * HALF_TILE_ROWS; e += blockDim.x) {
		const int c = e / HALF_TILE_ROWS, i = e - c * HALF_TILE_ROWS;
		if(i >= n_here)
			continue;
		const int64_t row = p_map? int64_t(p_map[r0 + i].x) : r0 + i;
		s_tile[i * HALF_TILE_LD + c] = (row >= 0)? p_cols[int64_t(c) * n_ld + row] : 0.0;
	}
	__syncthreads();
	for(int e = threadIdx.x; e < n_here * kp; e += blockDim.x) {
		const int i = e / kp, c = e - i * kp;
		p_inter[r0 * kp + e] = s_tile[i * HALF_TILE_LD + c];
	}
}

namespace {
enum { SOLVE_COLS_FORWARD = 1, SOLVE_COLS_BACKWARD = 2 }; // which substitutions a call of Solve_Columns_Passes runs
}

// The passes of slampp_hip_solve_columns (both halves: the forward substitution leaves y in the workspace, the backward one
// picks it up there) and of slampp_hip_solve_half_columns (one half: y leaves the workspace through half_export_kernel, or
// enters it through half_import_kernel; the substitutions' launches are the same ones in the same order).
static void Solve_Columns_Passes(slampp_hip_solver &s, double *p_rhs_dev, int64_t n_ld, int n_columns, int n_halves, const char *p_s_phase)
{
	const Plan &P = s.plan;
	CCovariance &cv = Covariance_State(s);
	if(!cv.b_columns)
		Setup_Columns(s, cv);
	if(!cv.b_solve_top)
		Setup_Solve_Top(s, cv);
	s.Ensure_Leaf_Inverses(); // (the substitutions multiply by inv(L_jj) of every column)
	const int D = Unrolled_Dim(P);
	const int n_per_wave = 64 / (D? D : 8);
	const int n_stages = int(P.stage_ptr.size()) - 1;
	const int ld = s.n_dense_pad, n_dense = s.n_dense_dim, n_tiles = ld / COV_NB;
	const bool b_forward = (n_halves & SOLVE_COLS_FORWARD) != 0, b_backward = (n_halves & SOLVE_COLS_BACKWARD) != 0;
	const unsigned n_row_tiles = unsigned((s.n_scalars + HALF_TILE_ROWS - 1) / HALF_TILE_ROWS);
	s.Phase_Begin(p_s_phase);
	for(int col0 = 0; col0 < n_columns; col0 += COV_K_PASS) {
		const int kp = std::min(int(COV_K_PASS), n_columns - col0);
		const unsigned n_groups = unsigned((kp + n_per_wave - 1) / n_per_wave);
		double *p_pass = p_rhs_dev + int64_t(col0) * n_ld;
#define SOLVE_COLS_DISPATCH(LAUNCH) switch(D) { case 3: LAUNCH(3); break; case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; default: LAUNCH(0); break; }
		for(int st = 0; b_forward && st < n_stages; ++ st) {
			const int n_tasks = P.stage_ptr[size_t(st + 1)] - P.stage_ptr[size_t(st)];
			if(n_tasks <= 0)
				continue;
#define SOLVE_COLS_FWD(DD) hipLaunchKernelGGL(solve_cols_forward_kernel<DD>, dim3(unsigned(n_tasks), n_groups), dim3(64), 0, s.stream, s.dplan.cols, \
				s.dplan.rents, s.dplan.task_ptr, P.stage_ptr[size_t(st)], s.d_L.p(), s.d_Linv.p(), p_pass, n_ld, cv.d_X.p(), kp)
			SOLVE_COLS_DISPATCH(SOLVE_COLS_FWD)
#undef SOLVE_COLS_FWD
		}
		if(n_dense && b_forward) {
			SLAMPP_HIP_CHECK(hipMemsetAsync(cv.d_Bd.p(), 0, size_t(ld) * kp * sizeof(double), s.stream)); // (gaps between the columns' positions)
			if(cv.n_top_cols) {
#define SOLVE_COLS_TOP(DD) hipLaunchKernelGGL(solve_cols_top_kernel<DD>, dim3(unsigned(cv.n_top_cols), n_groups), dim3(64), 0, s.stream, cv.d_top_cols.p(), \
				cv.d_top_ents.p(), s.d_L.p(), p_pass, n_ld, cv.d_X.p(), kp, cv.d_Bd.p())
				SOLVE_COLS_DISPATCH(SOLVE_COLS_TOP)
#undef SOLVE_COLS_TOP
			}
			for(int t = 0; t < n_tiles; ++ t)
				hipLaunchKernelGGL(cov_dense_forward_kernel, dim3(n_tiles - t), dim3(256), 0, s.stream, s.d_dense.p(), ld, n_dense, t,
					s.d_dense_invdiag.p(), cv.d_Bd.p(), cv.d_Zb.p(), kp);
		}
		if(!b_backward) { // y out: the block-eliminated rows from X (its dense-top rows hold nothing), then the top's from Zb over them
			hipLaunchKernelGGL(half_export_kernel, dim3(n_row_tiles), dim3(256), 0, s.stream, cv.d_X.p(), s.n_scalars, kp,
				(const longlong2*)0, p_pass, n_ld);
			if(n_dense)
				hipLaunchKernelGGL(half_export_kernel, dim3(unsigned(n_tiles)), dim3(256), 0, s.stream, cv.d_Zb.p(), int64_t(ld), kp,
					s.d_dense_dst.p(), p_pass, n_ld);
			continue;
		}
		if(!b_forward) { // y in: every row into X (the top's x replaces its rows there), the top's into Zb
			hipLaunchKernelGGL(half_import_kernel, dim3(n_row_tiles), dim3(256), 0, s.stream, p_pass, n_ld, s.n_scalars, kp,
				(const longlong2*)0, cv.d_X.p());
			if(n_dense)
				hipLaunchKernelGGL(half_import_kernel, dim3(unsigned(n_tiles)), dim3(256), 0, s.stream, p_pass, n_ld, int64_t(ld), kp,
					s.d_dense_dst.p(), cv.d_Zb.p());
		}
		if(n_dense) {
			for(int t = n_tiles - 1; t >= 0; -- t)
				hipLaunchKernelGGL(cov_dense_backward_kernel, dim3(t + 1), dim3(256), 0, s.stream, s.d_dense.p(), ld, n_dense, t,
					s.d_dense_invdiag.p(), cv.d_Zb.p(), kp, s.d_dense_dst.p(), cv.d_X.p(), p_pass, n_ld, 0);
		}
		for(int st = n_stages - 1; st >= 0; -- st) {
			const int n_tasks = P.stage_ptr[size_t(st + 1)] - P.stage_ptr[size_t(st)];
			if(n_tasks <= 0)
				continue;
#define SOLVE_COLS_BWD(DD) hipLaunchKernelGGL(solve_cols_backward_kernel<DD>, dim3(unsigned(n_tasks), n_groups), dim3(64), 0, s.stream, s.dplan.cols, \
				s.dplan.blks, s.dplan.task_ptr, P.stage_ptr[size_t(st)], s.d_L.p(), s.d_Linv.p(), cv.d_X.p(), kp, p_pass, n_ld)
			SOLVE_COLS_DISPATCH(SOLVE_COLS_BWD)
#undef SOLVE_COLS_BWD
		}
#undef SOLVE_COLS_DISPATCH
	}
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

void solve_columns_enqueue(slampp_hip_solver &s, double *p_rhs_dev, int64_t n_ld, int n_columns)
{
	Solve_Columns_Passes(s, p_rhs_dev, n_ld, n_columns, SOLVE_COLS_FORWARD | SOLVE_COLS_BACKWARD, "solve_columns");
}

void solve_half_columns_enqueue(slampp_hip_solver &s, bool b_backward, double *p_inout_dev, int64_t n_ld, int n_columns)
{
	Solve_Columns_Passes(s, p_inout_dev, n_ld, n_columns, b_backward? SOLVE_COLS_BACKWARD : SOLVE_COLS_FORWARD,
		b_backward? "solve_half_backward" : "solve_half_forward");
}

// ---- blocks at arbitrary pairs: Y_r^T Y_c over the rows the two paths share ----

enum { COV_GRAM_WAVES = 4 };

// One workgroup of COV_GRAM_WAVES waves per pair, lane e of every wave = output entry (a, b) = (e % dr, e / dr), at most 64.
// Wave w sums the listed columns w, w + COV_GRAM_WAVES, .. (each with its dim rows in order) and the w-th of COV_GRAM_WAVES
// contiguous chunks of the dense top's rows; the partial sums meet in LDS and are added in wave order: no atomics, every
// entry in one fixed order.  Reads rows of this pass's reach only (the listed ones; all of Zb is written in every pass
// that runs the dense tiles' forward substitution): X holds stale values elsewhere.
__global__ void __launch_bounds__(64 * COV_GRAM_WAVES)
cov_gram_kernel(const TPairRec *__restrict__ pairs, int64_t pair0, const TPairRow *__restrict__ rows, const double *__restrict__ X,
	const double *__restrict__ Zb, int n_dense, int kp, double *__restrict__ out)
{
	__shared__ double s_part[COV_GRAM_WAVES][64];
	const TPairRec rec = pairs[pair0 + blockIdx.x];
	const int e = threadIdx.x & 63, w = threadIdx.x >> 6;
	const bool b_act = e < rec.dr * rec.dc;
	const int la = b_act? rec.lane_r + e % rec.dr : 0, lb = b_act? rec.lane_c + e / rec.dr : 0; // (lanes < kp)
	double acc = 0;
	for(int q = w; q < rec.n_rows; q += COV_GRAM_WAVES) {
		const TPairRow row = rows[rec.row0 + q];
		const double *Xr = X + int64_t(row.cs) * kp;
		for(int t = 0; t < row.dim; ++ t)
			acc += Xr[t * kp + la] * Xr[t * kp + lb];
	}
	if(rec.dense) {
		const int n_chunk = (n_dense + COV_GRAM_WAVES - 1) / COV_GRAM_WAVES;
		const int i1 = (n_chunk * (w + 1) < n_dense)? n_chunk * (w + 1) : n_dense;
		#pragma unroll 4
		for(int i = n_chunk * w; i < i1; ++ i)
			acc += Zb[int64_t(i) * kp + la] * Zb[int64_t(i) * kp + lb];
	}
	s_part[w][e] = acc;
	__syncthreads();
	if(w == 0 && b_act) {
		double sum = s_part[0][e];
		#pragma unroll
		for(int v = 1; v < COV_GRAM_WAVES; ++ v)
			sum += s_part[v][e];
		out[rec.out + e] = sum;
	}
}

static void Gram_Enqueue(slampp_hip_solver &s, CCovariance &cv, const TPairPass &pass, int kp, double *p_out_dev)
{
	hipLaunchKernelGGL(cov_gram_kernel, dim3(unsigned(pass.pair1 - pass.pair0)), dim3(64 * COV_GRAM_WAVES), 0, s.stream,
		cv.d_pairs.p(), pass.pair0, cv.d_pair_rows.p(), cv.d_X.p(), cv.d_Zb.p(), s.n_dense_dim, kp, p_out_dev);
}

void covariance_pairs_enqueue(slampp_hip_solver &s, int64_t n_pairs, const int64_t *p_brows, const int64_t *p_bcols, double *p_out_dev)
{
	const Plan &P = s.plan;
	CCovariance &cv = Covariance_State(s);
	if(!cv.b_columns)
		Setup_Columns(s, cv);
	Lists_Begin(cv); // (before the pair records are touched: the previous call's uploads read them)
	plan_pairs(P, cv.sched_pos, n_pairs, p_brows, p_bcols, COV_K_PASS, cv.pair_plan);
	const PairPlan &pp = cv.pair_plan;
	cv.pairs = pp.pairs;
	cv.pair_rows = pp.rows;
	std::vector<TCovPass> passes(pp.passes.size());
	for(size_t p = 0; p < pp.passes.size(); ++ p) {
		passes[p].col0 = 0;
		passes[p].kp = pp.passes[p].kp;
		List_Pass(cv, P, int(pp.passes[p].cols.size()), pp.passes[p].cols.data(), pp.passes[p].lanes.data(), passes[p]);
	}
	Lists_Upload(s, cv);
	s.Phase_Begin("marginal_blocks");
	for(size_t p = 0; p < passes.size(); ++ p) {
		const TPairPass &pass = pp.passes[p];
		Forward_Enqueue(s, cv, passes[p], 0, pass.b_dense); // (no pair of the pass reaches the top: nobody reads d_Zb)
		Gram_Enqueue(s, cv, pass, passes[p].kp, p_out_dev);
	}
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

const PairPlan &covariance_pair_sets_plan(slampp_hip_solver &s, int64_t n_pairs, const int32_t *p_set_r, const int32_t *p_set_c,
	int32_t n_sets, const int64_t *p_set_ptr, const int32_t *p_set_src, const int32_t *p_set_width)
{
	const Plan &P = s.plan;
	CCovariance &cv = Covariance_State(s);
	if(!cv.b_columns)
		Setup_Columns(s, cv);
	Lists_Begin(cv); // (before the pair records are touched: the previous call's uploads read them)
	plan_pair_sets(P, cv.sched_pos, n_pairs, p_set_r, p_set_c, n_sets, p_set_ptr, p_set_src, p_set_width, COV_K_PASS, cv.pair_plan);
	const PairPlan &pp = cv.pair_plan;
	cv.pairs = pp.pairs;
	cv.pair_rows = pp.rows;
	cv.set_passes.assign(pp.passes.size(), TCovPass());
	for(size_t p = 0; p < pp.passes.size(); ++ p) {
		cv.set_passes[p].col0 = 0;
		cv.set_passes[p].kp = pp.passes[p].kp;
		List_Pass(cv, P, int(pp.passes[p].srcs.size()), pp.passes[p].srcs.data(), 0, cv.set_passes[p]);
	}
	Lists_Upload(s, cv);
	return pp;
}

void covariance_pair_sets_pass(slampp_hip_solver &s, size_t n_pass, const double *p_rhs_dev, double *p_out_dev)
{
	CCovariance &cv = Covariance_State(s);
	const TPairPass &pass = cv.pair_plan.passes.at(n_pass);
	Forward_Enqueue(s, cv, cv.set_passes.at(n_pass), p_rhs_dev, pass.b_dense);
	Gram_Enqueue(s, cv, pass, pass.kp, p_out_dev);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

void covariance_columns_enqueue(slampp_hip_solver &s, int n_cols, const int64_t *p_bcols, double *p_out_dev)
{
	columns_enqueue(s, n_cols, p_bcols, 0, 0, p_out_dev, s.n_scalars, 0);
}

void covariance_columns_rhs_enqueue(slampp_hip_solver &s, int n_src, const int64_t *p_src_bcols, int kp, const double *p_rhs_dev,
	double *p_out_dev, int64_t n_ld_out, int64_t n_col0)
{
	columns_enqueue(s, n_src, p_src_bcols, p_rhs_dev, kp, p_out_dev, n_ld_out, n_col0);
}

} // namespace slampp
