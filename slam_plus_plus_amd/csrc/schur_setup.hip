// schur_setup.hip -- the host side of the BA path's set-up, no kernel: the analysis of a system's structure (observation
// lists, the blocks of S and their contribution lists or tiles), the exchange in which landmark shards agree on the blocks
// of S, the choice and construction of the inner sparse solver for the reduced camera system, the tables the covariances
// read the sparse inverse subset through, and the small functions on CSchurState.
#include "schur_state.h"
#include "dense_chol.h"
#include "covariance.h"
#include "host_threads.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace slampp {

static double schur_wall_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

CSchurState::~CSchurState()
{
	if(p_sinv)
		sparse_inverse_destroy(p_sinv);
	for(int i = 0; i < 2; ++ i) {
		if(ev_cov_cols[i])
			(void)hipEventDestroy(ev_cov_cols[i]);
	}
	if(p_inner) {
		p_inner->stream = 0; // borrowed from the owning solver
		delete p_inner;
	}
}

void schur_destroy(CSchurState *p) { delete p; }

size_t schur_device_bytes(const CSchurState *p)
{
	return p->d_ptr.n_Bytes() + p->d_brow.n_Bytes() + p->d_obs_pt.n_Bytes() + p->d_sb_ptr.n_Bytes() +
		p->d_sb_row.n_Bytes() + p->d_sb_col.n_Bytes() + p->d_ent_a.n_Bytes() + p->d_ent_uoff.n_Bytes() +
		p->d_cam_ptr.n_Bytes() + p->d_cam_obs.n_Bytes() + p->d_S.n_Bytes() + p->d_W.n_Bytes() +
		p->d_un_row.n_Bytes() + p->d_un_col.n_Bytes() + p->d_pack.n_Bytes() + p->d_sb_dst.n_Bytes() + p->d_a_dst.n_Bytes() +
		p->d_in_buf.n_Bytes() + (p->p_inner? p->p_inner->n_Device_Bytes() : 0) + p->d_m_S.n_Bytes() + p->d_m_Z.n_Bytes() +
		p->d_m_invdiag.n_Bytes() + p->d_m_zero.n_Bytes() + p->d_m_Zs.n_Bytes() + p->d_cam_zoff.n_Bytes() +
		p->d_pair_ptr.n_Bytes() + p->d_pair_tab.n_Bytes() + sparse_inverse_bytes(p->p_sinv) +
		p->d_Cinv.n_Bytes() + p->d_t.n_Bytes() + p->d_invdiag.n_Bytes() + p->d_z.n_Bytes() + p->d_x.n_Bytes() +
		p->d_A_prev.n_Bytes() + p->d_S_unf.n_Bytes() + p->d_changed.n_Bytes() + p->tiles.n_Bytes() + p->d_a_zent.n_Bytes() +
		p->d_cam_csn.n_Bytes() + p->d_cov_cols.n_Bytes() + p->d_cov_B.n_Bytes() + p->d_cov_X.n_Bytes() + p->d_cov_pairs.n_Bytes();
}

void schur_invalidate_previous(CSchurState *p)
{
	if(p) {
		p->b_prev_valid = false;
		p->n_changed = -1;
	}
}

// names the landmarks whose blocks differ from the previous solve's (host list, strictly increasing)
void schur_set_changed_points(slampp_hip_solver &s, const int64_t *p_points, int64_t n_points)
{
	CSchurState &S = *s.p_schur;
	for(int64_t i = 0; i < n_points; ++ i) {
		if(p_points[i] < 0 || p_points[i] >= S.np || (i && p_points[i] <= p_points[i - 1]))
			throw std::invalid_argument("schur_set_changed_points: landmark indices must be strictly increasing and in range");
	}
	S.d_changed.Alloc(size_t(std::max<int64_t>(n_points, 1)));
	if(n_points)
		SLAMPP_HIP_CHECK(hipMemcpy(S.d_changed.p(), p_points, size_t(n_points) * sizeof(int64_t), hipMemcpyHostToDevice));
	S.n_changed = n_points;
}

// stats of the inner solver that factors the reduced camera system by the sparse block path; false while there is none
// (dense reduced system, or no solve has decided yet)
bool schur_reduced_stats(const CSchurState *p, slampp_hip_stats &st)
{
	return p && p->b_reduced_decided && p->b_reduced_sparse && p->p_inner && slampp_hip_get_stats(p->p_inner, &st) == SLAMPP_HIP_OK;
}

void schur_fill_stats(const CSchurState *p, slampp_hip_stats &st)
{
	st.n_cams = p->nc;
	st.n_points = p->np;
	st.n_observations = p->n_obs;
	st.schur_dim = p->N;
	st.n_update_pairs = p->n_entries;
	st.l_blocks = p->n_sblocks;
	const double n = double(p->N);
	st.factor_flops = n * n * n / 3.0 + n * (n - 1) / 2.0 + n; // dense Cholesky (slam_schur_orderings/Main.cpp:682)
	st.solve_flops = 2.0 * n * n;
}

// ---------------------------------------------------------------------------------------------
// host analysis
// ---------------------------------------------------------------------------------------------

CSchurState *schur_analyze(slampp_hip_solver &s)
{
	const int64_t n = int64_t(s.cumsum.size()) - 1, nc = s.n_matrix_cut, np = n - nc;
	const int64_t *cs = s.cumsum.data(), *ptr = s.bcol_ptr.data();
	const int32_t *brow = s.brow.data();
	const int64_t DC = cs[1] - cs[0], DP = cs[nc + 1] - cs[nc];
	{
		// the shape of the system, column by column -- on a few threads from 65 536 block columns on (round 6: two passes over
		// C5's two million columns were 5 - 7 ms on one); what is reported is what the serial passes reported: a block size out of
		// line first, then the first landmark that is wrong and how, then the first camera
		const int n_check_threads = host_thread_count(n, 16384, 4); // (four from 65 536 block columns on)
		struct TFirst { int64_t n_size, n_landmark, n_camera; int n_landmark_error; };
		std::vector<TFirst> first(size_t(n_check_threads), TFirst{-1, -1, -1, 0});
		for_ranges(0, n, n_check_threads, [&](int t, int64_t c0, int64_t c1) {
			TFirst &r_first = first[size_t(t)];
			for(int64_t c = c0; c < c1; ++ c) {
				if(r_first.n_size < 0 && cs[c + 1] - cs[c] != (c < nc? DC : DP))
					r_first.n_size = c;
				const bool b_no_diagonal = ptr[c + 1] == ptr[c] || brow[ptr[c + 1] - 1] != c;
				if(c < nc) {
					if(r_first.n_camera < 0 && b_no_diagonal)
						r_first.n_camera = c;
				} else if(r_first.n_landmark < 0) {
					if(b_no_diagonal) {
						r_first.n_landmark = c;
						r_first.n_landmark_error = 1;
					} else if(ptr[c + 1] - ptr[c] >= 2 && brow[ptr[c + 1] - 2] >= nc) {
						r_first.n_landmark = c;
						r_first.n_landmark_error = 2;
					}
				}
			}
		});
		for(int t = 0; t < n_check_threads; ++ t) {
			if(first[size_t(t)].n_size >= 0)
				throw std::domain_error("Schur path: cameras and landmarks must each have one block size");
		}
		if(!((DC == 6 && DP == 3) || (DC == 7 && DP == 3) || (DC == 3 && DP == 2)))
			throw std::domain_error("Schur path: supported (camera, landmark) block sizes are (6,3), (7,3), (3,2)");
		for(int t = 0; t < n_check_threads; ++ t) { // (the threads' ranges ascend: the first one with a complaint has the first landmark)
			if(first[size_t(t)].n_landmark_error == 1)
				throw std::invalid_argument("Schur path: a landmark has no diagonal block");
			if(first[size_t(t)].n_landmark_error == 2)
				throw std::domain_error("Schur path: landmark-landmark blocks present, C is not block diagonal");
		}
		for(int t = 0; t < n_check_threads; ++ t) {
			if(first[size_t(t)].n_camera >= 0)
				throw std::invalid_argument("Schur path: a camera has no diagonal block");
		}
	}
	if(nc * DC + 64 > INT32_MAX / 2)
		throw std::domain_error("Schur path: reduced system too large");

	CSchurState *p = new CSchurState();
	try {
		CSchurState &S = *p;
		S.DC = int(DC); S.DP = int(DP);
		S.nc = nc; S.np = np;
		S.n_ablocks = ptr[nc];
		S.n_obs = ptr[n] - ptr[nc] - np;
		S.N = int(nc * DC);
		S.Npad = dense_padded_dim(S.N);
		if(S.n_obs > INT32_MAX)
			throw std::domain_error("Schur path: too many observations");

		const bool b_timing = getenv("SLAMPP_HIP_PLAN_TIMING") != 0;
		double t_phase = schur_wall_ms();
#define SCHUR_SETUP_PHASE(name) do { if(b_timing) { const double t_ = schur_wall_ms(); \
		fprintf(stderr, "[schur setup] %-20s %8.2f ms\n", name, t_ - t_phase); t_phase = t_; } } while(0)
		// (round 4: the passes over the landmarks run on a few threads, a range of landmarks each -- C5's two million landmarks
		// and eight million observations were 34 + 19 ms here on one core; the camera-major list is a counting sort with one
		// counter array per thread, so every observation still lands where the serial pass put it)
		const int n_setup_workers = host_thread_count(np, 65536);
		raw_vector<int32_t> obs_pt(S.n_obs), obs_cam(S.n_obs); // (written in full by the pass below)
		std::vector<int64_t> cam_ptr(nc + 1, 0);
		std::vector<std::vector<int64_t> > cam_count(n_setup_workers, std::vector<int64_t>(size_t(nc), 0));
		for_ranges(0, np, n_setup_workers, [&](int t, int64_t n_first, int64_t n_last) {
			std::vector<int64_t> &r_count = cam_count[t];
			for(int64_t pt = n_first; pt < n_last; ++ pt) {
				const int64_t c = nc + pt, o0 = ptr[c] - ptr[nc] - pt;
				for(int64_t k = ptr[c]; k < ptr[c + 1] - 1; ++ k) {
					const int64_t o = o0 + (k - ptr[c]);
					obs_pt[o] = int32_t(pt);
					obs_cam[o] = brow[k];
					++ r_count[brow[k]];
				}
			}
		});
		for(int64_t c = 0; c < nc; ++ c) { // per camera: where each thread's observations start (threads in landmark order)
			int64_t n_sum = cam_ptr[c];
			for(int t = 0; t < n_setup_workers; ++ t) {
				const int64_t n_here = cam_count[t][c];
				cam_count[t][c] = n_sum;
				n_sum += n_here;
			}
			cam_ptr[c + 1] = n_sum;
		}
		raw_vector<int32_t> cam_obs(S.n_obs);
		for_ranges(0, np, n_setup_workers, [&](int t, int64_t n_first, int64_t n_last) {
			std::vector<int64_t> &r_fill = cam_count[t];
			const int64_t o_first = ptr[nc + n_first] - ptr[nc] - n_first, o_last = ptr[nc + n_last] - ptr[nc] - n_last;
			for(int64_t o = o_first; o < o_last; ++ o)
				cam_obs[r_fill[obs_cam[o]] ++] = int32_t(o);
		});
		SCHUR_SETUP_PHASE("observation lists");
		// what is ready goes to the device from here on, beside the rest of the analysis (round 6: 130 MB out of pageable
		// vectors at C5, 7 ms at the end of the analysis; the vectors are not written again, and joined before the final sync)
		std::exception_ptr p_early_upload_error;
		CJoinedThread t_early_upload;
		s.Join_Bringup(); // (a handle fresh from slampp_hip_create: its streams came up beside the checks and the observation lists -- solver.h)
		{
			const int n_device = s.n_device;
			hipStream_t st_early = s.stream;
			auto Early_Uploads = [&, n_device, st_early]() {
				try {
					SLAMPP_HIP_CHECK(hipSetDevice(n_device));
					S.d_ptr.Upload(s.bcol_ptr, st_early);
					S.d_brow.Upload(s.brow, st_early);
					S.d_obs_pt.Upload(obs_pt, st_early);
					S.d_cam_ptr.Upload(cam_ptr, st_early);
					S.d_cam_obs.Upload(cam_obs, st_early);
				} catch(...) {
					p_early_upload_error = std::current_exception();
				}
			};
			if(S.n_obs >= (int64_t(1) << 20))
				t_early_upload.t = std::thread(Early_Uploads);
			else
				Early_Uploads(); // (a small system: a thread's start-up is what it would save)
		}
		// contributions to S grouped by block (row = camera of b, col = camera of a, a <= b within a point)
		// (the builders of schur_tile_tables.cpp)
		std::vector<int64_t> sb_ptr;
		std::vector<int32_t> sb_row, sb_col;
		raw_vector<int32_t> ent_a;    // (the contribution lists -- 5 M entries at the uniform-visibility C4 -- and the counters they are
		raw_vector<int64_t> ent_uoff; // placed with: mappings of the library's own on huge pages, host_pool.h)
		bool b_tiles_built = false;
		{
			int64_t n_entries = 0;
			for(int64_t pt = 0; pt < np; ++ pt) {
				const int64_t k = ptr[nc + pt + 1] - ptr[nc + pt] - 1;
				n_entries += k * (k + 1) / 2;
			}
			S.n_entries = n_entries;
			const SchurStructure t_structure = {int(DC), int(DP), nc, np, ptr, brow, S.n_ablocks};
			if(nc * nc <= (int64_t(1) << 26)) { // the dense key space
				schur_blocks_from_bitmap(sb_row, sb_col, t_structure, obs_cam, n_setup_workers);
				SCHUR_SETUP_PHASE("blocks of S");
				// the blocks of S are known: can the landmarks be taken one by one (schur_tiles.hip)?  Then the per-block
				// contribution lists -- 12 bytes and a scattered write per contribution -- are not needed at all
				schur_tiles_build(S.tiles, s.n_schur_tiles, int(DC), int(DP), nc, np, ptr, brow, sb_row, sb_col, S.n_ablocks, s.stream);
				b_tiles_built = true;
				SCHUR_SETUP_PHASE("runs and tiles");
				if(!S.tiles.b_enabled) // the lists of every block after all
					schur_lists_by_counting(sb_ptr, ent_a, ent_uoff, t_structure, obs_cam, n_entries, sb_row.size(), n_setup_workers);
			} else
				schur_lists_by_sorting(sb_ptr, sb_row, sb_col, ent_a, ent_uoff, t_structure, obs_cam, obs_pt, n_entries);
		}
		S.n_sblocks = int64_t(sb_row.size());
		S.h_blk_row = sb_row;
		S.h_blk_col = sb_col;
		for(int64_t c = 0; c < nc; ++ c) { // the camera-camera blocks of Lambda land in S too (transposed: lower triangle)
			for(int64_t k = ptr[c]; k < ptr[c + 1]; ++ k) {
				S.h_blk_row.push_back(int32_t(c));
				S.h_blk_col.push_back(brow[k]);
			}
		}

		SCHUR_SETUP_PHASE("contribution lists");
		hipStream_t st = s.stream;
		if(!b_tiles_built)
			schur_tiles_build(S.tiles, s.n_schur_tiles, int(DC), int(DP), nc, np, ptr, brow, sb_row, sb_col, S.n_ablocks, st);
		SCHUR_SETUP_PHASE("runs and tiles");
		S.d_sb_ptr.Upload(sb_ptr, st);
		S.d_sb_row.Upload(sb_row, st);
		S.d_sb_col.Upload(sb_col, st);
		S.d_ent_a.Upload(ent_a, st);
		S.d_ent_uoff.Upload(ent_uoff, st);
		if(t_early_upload.t.joinable())
			t_early_upload.t.join();
		if(p_early_upload_error)
			std::rethrow_exception(p_early_upload_error);
		S.d_W.Alloc(size_t(S.n_obs) * (DC * DP));
		S.d_Cinv.Alloc(size_t(np) * DP * DP);
		S.d_t.Alloc(size_t(S.n_obs) * DP);
		s.d_flag.Alloc(1);
		SLAMPP_HIP_CHECK(hipMemsetAsync(s.d_flag.p(), 0, sizeof(int), s.stream)); // sync() before the first factorization reads it
		schur_tiles_join(S.tiles); // (the run tables, uploaded beside everything since the runs were found)
		SLAMPP_HIP_CHECK(hipStreamSynchronize(st));
		SCHUR_SETUP_PHASE("uploads");
		if(S.n_obs >= (int64_t(1) << 20) || !S.tiles.trash.empty()) {
			// the observation lists are on the device: their memory (C5: 100 MB) goes back to the system on a thread behind the
			// analysis' return, not at the end of this scope (solver.h: TTrash, t_discard)
			s.Join_Discard();
			for(size_t i = 0; i < S.tiles.trash.size(); ++ i)
				s.analysis_trash.emplace_back(std::move(S.tiles.trash[i])); // (the tile analysis' hashes, sort items and orders)
			S.tiles.trash.clear();
			Discard_Later(s.analysis_trash, obs_pt); Discard_Later(s.analysis_trash, obs_cam); Discard_Later(s.analysis_trash, cam_obs);
			Discard_Later(s.analysis_trash, ent_a); Discard_Later(s.analysis_trash, ent_uoff);
			slampp_hip_solver *p_solver = &s;
			try {
				s.t_discard = std::thread([p_solver]() { p_solver->analysis_trash.clear(); host_pool_release(); });
			} catch(std::system_error&) {
				s.analysis_trash.clear();
				host_pool_release();
			}
		}
#undef SCHUR_SETUP_PHASE
	} catch(...) {
		delete p;
		throw;
	}
	return p;
}

// Agrees with the other ranks on the set of blocks to exchange, through the caller's sum all-reduce alone: with
// "shard_rank" / "shard_world" set, the ranks concatenate their block lists (each writes into its own slot of a
// zeroed buffer); without, every rank marks its blocks in an indicator over the lower triangle of the camera-block
// grid.  Either way every rank derives the same ordered list from the sum.  One-time, synchronous.
void schur_agree_on_union(slampp_hip_solver &s, CSchurState &S)
{
	hipStream_t st = s.stream;
	S.p_union_fn = s.p_allreduce;
	S.p_union_context = s.p_allreduce_context;
	S.n_union = 0;
	S.h_un_row.clear();
	S.h_un_col.clear();
	S.b_reduced_decided = false; // the block list the sparse reduced system is built from may change
	const int64_t nc = S.nc;
	std::vector<int32_t> un_row, un_col;
	// this rank's blocks as sorted, unique keys col * nc + row
	std::vector<int64_t> own(S.h_blk_row.size());
	for(size_t i = 0; i < own.size(); ++ i)
		own[i] = int64_t(S.h_blk_col[i]) * nc + S.h_blk_row[i];
	std::sort(own.begin(), own.end());
	own.erase(std::unique(own.begin(), own.end()), own.end());
	const int n_world = s.n_shard_world, n_rank = s.n_shard_rank;
	S.b_union_dense = false;
	if(n_world > 0 && n_rank >= 0 && n_rank < n_world) {
		// the caller told us who we are: every rank writes its list into its own slot of a zeroed buffer and the sum
		// is the concatenation -- the exchange grows with the number of nonzero blocks, not with nc^2
		std::vector<double> len(size_t(n_world), 0.0);
		len[n_rank] = double(own.size());
		CDevArray<double> d_len;
		d_len.Alloc(size_t(n_world));
		SLAMPP_HIP_CHECK(hipMemcpyAsync(d_len.p(), len.data(), len.size() * sizeof(double), hipMemcpyHostToDevice, st));
		if(s.p_allreduce(s.p_allreduce_context, d_len.p(), len.size(), (void*)st) != 0)
			throw CDeviceError("all-reduce callback failed");
		SLAMPP_HIP_CHECK(hipMemcpyAsync(len.data(), d_len.p(), len.size() * sizeof(double), hipMemcpyDeviceToHost, st));
		SLAMPP_HIP_CHECK(hipStreamSynchronize(st));
		size_t n_total = 0, n_before = 0;
		for(int r = 0; r < n_world; ++ r) {
			if(r == n_rank)
				n_before = n_total;
			n_total += size_t(len[r]);
		}
		if(size_t(len[n_rank]) != own.size())
			throw std::invalid_argument("shard_rank / shard_world do not match the ranks behind the all-reduce callback");
		std::vector<double> all(n_total, 0.0);
		for(size_t i = 0; i < own.size(); ++ i)
			all[n_before + i] = double(own[i]); // exact: keys are below 2^53
		CDevArray<double> d_all;
		d_all.Alloc(n_total);
		SLAMPP_HIP_CHECK(hipMemcpyAsync(d_all.p(), all.data(), n_total * sizeof(double), hipMemcpyHostToDevice, st));
		if(s.p_allreduce(s.p_allreduce_context, d_all.p(), n_total, (void*)st) != 0)
			throw CDeviceError("all-reduce callback failed");
		SLAMPP_HIP_CHECK(hipMemcpyAsync(all.data(), d_all.p(), n_total * sizeof(double), hipMemcpyDeviceToHost, st));
		SLAMPP_HIP_CHECK(hipStreamSynchronize(st));
		std::vector<int64_t> keys(n_total);
		for(size_t i = 0; i < n_total; ++ i)
			keys[i] = int64_t(all[i]);
		std::sort(keys.begin(), keys.end());
		keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
		for(size_t i = 0; i < keys.size(); ++ i) {
			if(keys[i] < 0 || keys[i] >= nc * nc || keys[i] % nc < keys[i] / nc)
				throw std::invalid_argument("block-list exchange returned an impossible key: is the callback a sum over all ranks?");
			un_col.push_back(int32_t(keys[i] / nc));
			un_row.push_back(int32_t(keys[i] % nc));
		}
	} else {
		// ranks unknown: an indicator over the lower triangle of the camera-block grid, summed
		S.b_union_dense = S.nc > 16384; // the indicator would exceed a gigabyte
		if(S.b_union_dense)
			return;
		const int64_t n_tri = nc * (nc + 1) / 2;
		std::vector<double> ind(size_t(n_tri), 0.0);
		for(size_t i = 0; i < own.size(); ++ i) {
			const int64_t c = own[i] / nc, r = own[i] % nc;
			ind[size_t(c * nc - c * (c - 1) / 2 + (r - c))] = 1.0;
		}
		CDevArray<double> d_ind;
		d_ind.Alloc(size_t(n_tri));
		SLAMPP_HIP_CHECK(hipMemcpyAsync(d_ind.p(), ind.data(), size_t(n_tri) * sizeof(double), hipMemcpyHostToDevice, st));
		if(s.p_allreduce(s.p_allreduce_context, d_ind.p(), size_t(n_tri), (void*)st) != 0)
			throw CDeviceError("all-reduce callback failed");
		SLAMPP_HIP_CHECK(hipMemcpyAsync(ind.data(), d_ind.p(), size_t(n_tri) * sizeof(double), hipMemcpyDeviceToHost, st));
		SLAMPP_HIP_CHECK(hipStreamSynchronize(st));
		size_t k = 0;
		for(int64_t c = 0; c < nc; ++ c) {
			for(int64_t r = c; r < nc; ++ r, ++ k) {
				if(ind[k] > 0.5) {
					un_row.push_back(int32_t(r));
					un_col.push_back(int32_t(c));
				}
			}
		}
	}
	S.n_union = int64_t(un_row.size());
	S.h_un_row = un_row;
	S.h_un_col = un_col;
	S.d_un_row.Upload(un_row, st);
	S.d_un_col.Upload(un_col, st);
	SLAMPP_HIP_CHECK(hipStreamSynchronize(st)); // un_row / un_col live on this stack frame
}

// Decides how the reduced camera system is factored and, for the sparse choice, builds the inner solver: S becomes
// a block matrix with one block column per camera whose structure is the block list every rank agreed on (or this
// rank's own list on a single GPU), analyzed once by the same ordering / symbolic / scheduling code as a pose graph.
static void schur_try_sparse_reduced(slampp_hip_solver &s, CSchurState &S)
{
	S.b_reduced_sparse = false;
	if(S.p_sinv) { // lists of the previous inner solver
		sparse_inverse_destroy(S.p_sinv);
		S.p_sinv = 0;
	}
	S.b_sinv_tried = false;
	S.d_a_zent.Free(); // (the covariance tables point into the previous inner solver's factor: built again on first use)
	S.d_cam_csn.Free();
	S.b_cov_z_valid = false;
	if(S.p_inner) {
		S.p_inner->stream = 0;
		delete S.p_inner;
		S.p_inner = 0;
	}
	if(s.n_schur_sparse == 0 || (s.p_allreduce && S.b_union_dense))
		return;
	std::vector<int32_t> rows, cols;
	if(s.p_allreduce) {
		rows = S.h_un_row;
		cols = S.h_un_col;
	} else {
		std::vector<int64_t> keys(S.h_blk_row.size());
		for(size_t i = 0; i < keys.size(); ++ i)
			keys[i] = int64_t(S.h_blk_col[i]) * S.nc + S.h_blk_row[i];
		std::sort(keys.begin(), keys.end());
		keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
		rows.resize(keys.size());
		cols.resize(keys.size());
		for(size_t i = 0; i < keys.size(); ++ i) {
			cols[i] = int32_t(keys[i] / S.nc);
			rows[i] = int32_t(keys[i] % S.nc);
		}
	}
	const int64_t nc = S.nc, n_list = int64_t(rows.size());
	const double f_fill = double(n_list) / (0.5 * double(nc) * double(nc + 1));
	// measured (Venice-like visibility, 300k landmarks): 3 % of the blocks nonzero 6.6 against 17.7 ms, 6 % (C4's Venice leg)
	// 3.6 against 5.2, 12 % 1.8 against 2.3, 20 % 1.74 against 1.69, every pair (uniform) 5.7 against 5.4
	if(s.n_schur_sparse < 0 && !(nc >= 128 && f_fill < 0.15))
		return; // dense: the MFMA factorization wins once S is effectively dense
	// upper block-CSC: the lower block (r, c) is the transpose of the upper block (c, r) in block column r
	std::vector<int64_t> cumsum(nc + 1), bcol_ptr(nc + 1, 0);
	for(int64_t c = 0; c <= nc; ++ c)
		cumsum[c] = c * S.DC;
	for(int64_t i = 0; i < n_list; ++ i)
		++ bcol_ptr[rows[i] + 1];
	for(int64_t c = 0; c < nc; ++ c)
		bcol_ptr[c + 1] += bcol_ptr[c];
	std::vector<int32_t> brow(n_list);
	std::vector<int64_t> in_off(n_list);
	{
		std::vector<int64_t> fill(bcol_ptr.begin(), bcol_ptr.end() - 1);
		for(int64_t i = 0; i < n_list; ++ i) { // the list is sorted by (col, row): within a block column the rows come out ascending
			const int64_t k = fill[rows[i]] ++;
			brow[k] = cols[i];
			in_off[i] = k * S.DC * S.DC;
		}
	}
	for(int64_t c = 0; c < nc; ++ c) {
		if(bcol_ptr[c + 1] == bcol_ptr[c] || brow[bcol_ptr[c + 1] - 1] != c)
			throw std::logic_error("reduced camera system: a camera has no diagonal block");
	}
	slampp_hip_solver *p_inner = new slampp_hip_solver();
	S.p_inner = p_inner;
	p_inner->n_device = s.n_device;
	p_inner->stream = s.stream; // borrowed
	p_inner->opt = s.opt;
	p_inner->n_simt = s.n_simt;
	p_inner->n_simt_width = s.n_simt_width;
	p_inner->n_simt_stages = s.n_simt_stages;
	p_inner->n_wide_min_tasks = s.n_wide_min_tasks;
	p_inner->n_panel_rows = s.n_panel_rows;
	p_inner->n_panel_backward = s.n_panel_backward;
	p_inner->n_panel_handup = s.n_panel_handup;
	p_inner->n_dense_top_tiles = s.n_dense_top_tiles;
	// (a small system is all latency: round 1 cut its leaf subtrees to four columns for the wave-per-task kernel; as panels
	// -- eight waves per subtree, 2 us per column -- the default of eight is faster again: 0.231 -> 0.220 ms at 1000 cameras)
	p_inner->cumsum = cumsum;
	p_inner->bcol_ptr = bcol_ptr;
	p_inner->brow = brow;
	p_inner->n_values = n_list * S.DC * S.DC;
	p_inner->n_scalars = nc * S.DC;
	p_inner->b_has_structure = true;
	p_inner->n_mode = SLAMPP_HIP_MODE_SPARSE;
	p_inner->Analyze_Sparse();
	p_inner->b_analyzed = true;
	S.n_in_blocks = n_list;
	// where this rank's own blocks go: the list is sorted by (col, row)
	std::vector<int64_t> keys(n_list);
	for(int64_t i = 0; i < n_list; ++ i)
		keys[i] = int64_t(cols[i]) * nc + rows[i];
	const size_t n_own = S.h_blk_row.size() - size_t(S.n_ablocks); // h_blk = [blocks of the gather | camera blocks of Lambda]
	std::vector<int64_t> sb_dst(n_own), a_dst(S.n_ablocks);
	for(size_t i = 0; i < S.h_blk_row.size(); ++ i) {
		const int64_t key = int64_t(S.h_blk_col[i]) * nc + S.h_blk_row[i];
		const size_t k = size_t(std::lower_bound(keys.begin(), keys.end(), key) - keys.begin());
		if(k == keys.size() || keys[k] != key)
			throw std::logic_error("reduced camera system: a block of this rank is missing from the agreed list");
		((i < n_own)? sb_dst[i] : a_dst[i - n_own]) = in_off[k];
	}
	S.d_sb_dst.Upload(sb_dst, s.stream);
	S.d_a_dst.Upload(a_dst, s.stream);
	S.d_in_buf.Alloc(size_t(n_list) * S.DC * S.DC + size_t(S.N));
	SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream)); // the host vectors live on this stack frame
	S.b_reduced_sparse = true;
}

void schur_setup_reduced(slampp_hip_solver &s, CSchurState &S)
{
	schur_try_sparse_reduced(s, S);
	if(!S.b_reduced_sparse) { // the dense buffers are only needed now
		S.d_S.Alloc(size_t(S.Npad) * S.Npad);
		S.d_invdiag.Alloc(size_t(S.Npad / dense_NB) * dense_NB * dense_NB);
		S.d_z.Alloc(S.Npad);
		S.d_x.Alloc(S.Npad);
		if(s.p_allreduce && !S.b_union_dense)
			S.d_pack.Alloc(size_t(S.n_union) * S.DC * S.DC + size_t(S.N));
	}
	S.b_reduced_decided = true;
}

// lists of the sparse inverse subset and the tables that say where the blocks the covariances need sit in it; false if
// the inner solver's plan is not of the kind sparse_inverse_setup takes (then the dense inverse is used)
bool schur_setup_sparse_marginals(slampp_hip_solver &s, CSchurState &S)
{
	if(S.b_sinv_tried)
		return S.p_sinv != 0;
	S.b_sinv_tried = true;
	const Plan &P = S.p_inner->plan;
	if(P.max_dim != S.DC)
		return false;
	S.p_sinv = sparse_inverse_setup(P, s.stream);
	if(!S.p_sinv)
		return false;
	const int64_t nc = S.nc, np = S.np;
	const int64_t *ptr = s.bcol_ptr.data();
	const int32_t *brow = s.brow.data();
	std::vector<int64_t> cam_zoff(nc), pair_ptr(np + 1, 0);
	for(int64_t c = 0; c < nc; ++ c)
		cam_zoff[c] = P.loff[P.lptr[P.pinv[c]]];
	for(int64_t pt = 0; pt < np; ++ pt) {
		const int64_t k = ptr[nc + pt + 1] - ptr[nc + pt] - 1;
		pair_ptr[pt + 1] = pair_ptr[pt] + k * (k + 1) / 2;
	}
	std::vector<int64_t> pair_tab((size_t(pair_ptr[np])));
	for(int64_t pt = 0; pt < np; ++ pt) {
		const int64_t k0 = ptr[nc + pt], k = ptr[nc + pt + 1] - k0 - 1;
		int64_t *tab = pair_tab.data() + pair_ptr[pt];
		for(int64_t a = 0; a < k; ++ a) {
			const int32_t pa = P.pinv[brow[k0 + a]];
			for(int64_t b = 0; b <= a; ++ b) {
				const int32_t pb = P.pinv[brow[k0 + b]];
				const int64_t off = plan_block_offset(P, std::max(pa, pb), std::min(pa, pb));
				if(off < 0)
					throw std::logic_error("covariances: a camera pair that shares a landmark is not a block of the reduced system's factor");
				tab[a * (a + 1) / 2 + b] = off * 2 + (pa < pb); // Z(cam_a, cam_b) is the stored block, or its transpose
			}
		}
	}
	S.d_cam_zoff.Upload(cam_zoff, s.stream);
	S.d_pair_ptr.Upload(pair_ptr, s.stream);
	S.d_pair_tab.Upload(pair_tab, s.stream);
	S.d_m_Zs.Alloc(size_t(P.loff.back()));
	if(!S.d_m_zero.p()) {
		const size_t n_zero = size_t(S.N) + size_t(S.np) * S.DP; // a whole right-hand side of zeros (the assembly reads the landmarks' part too)
		S.d_m_zero.Alloc(n_zero);
		SLAMPP_HIP_CHECK(hipMemsetAsync(S.d_m_zero.p(), 0, n_zero * sizeof(double), s.stream));
	}
	SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream)); // the tables live on this stack frame
	return true;
}

// the sparse path's extra tables: where Z(r, c) of every camera block of A sits in the inverse subset (A's blocks are blocks
// of S, so of its factor), and every camera's first row in the inner solver's permuted vector
void schur_setup_cov_tables(slampp_hip_solver &s, CSchurState &S)
{
	if(S.d_cam_csn.p())
		return;
	const Plan &P = S.p_inner->plan;
	const int64_t nc = S.nc, *ptr = s.bcol_ptr.data();
	const int32_t *brow = s.brow.data();
	std::vector<int64_t> a_zent(size_t(std::max<int64_t>(ptr[nc], 1)), int64_t(0)), cam_csn((size_t(nc)));
	for(int64_t c = 0; c < nc; ++ c) {
		const int32_t pc = P.pinv[size_t(c)];
		cam_csn[size_t(c)] = P.cs_new[size_t(pc)];
		for(int64_t k = ptr[c]; k < ptr[c + 1]; ++ k) {
			const int32_t pr = P.pinv[size_t(brow[k])];
			const int64_t off = plan_block_offset(P, std::max(pr, pc), std::min(pr, pc));
			if(off < 0)
				throw std::logic_error("covariances: a camera block of Lambda is not a block of the reduced system's factor");
			a_zent[size_t(k)] = off * 2 + (pr < pc); // Z(r, c) is the stored block, or its transpose
		}
	}
	S.d_a_zent.Upload(a_zent, s.stream);
	S.d_cam_csn.Upload(cam_csn, s.stream);
	SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream)); // the tables live on this stack frame
}

} // namespace slampp
