// schur_tile_tables_driver.cpp -- the host builders of the BA analysis (csrc/schur_tile_tables.cpp) on the CPU: a program
// of its own, built by tests/test_schur_tile_tables_sanitizers.py with g++ under sanitizers.  For each case it builds a BA
// structure, runs the builders in the analysis' order and decodes every table again against a brute-force walk of the
// landmarks' camera lists.  One line per case: "name: reached <branches> ok".  With the argument "threads" only the
// many-worker cases run (the ThreadSanitizer build).
#include "schur_tile_tables.h"

#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <random>
#include <set>
#include <stdexcept>
#include <string>

using namespace slampp;

typedef std::vector<std::vector<int32_t> > CLists; // the cameras of every landmark, ascending

struct TCheckFailed : std::runtime_error { using std::runtime_error::runtime_error; };
#define CHECK(cond) do { if(!(cond)) throw TCheckFailed(std::string(#cond) + " (line " + std::to_string(__LINE__) + ")"); } while(0)

struct TStructure { // cameras with a diagonal block each, then the landmarks' columns [cameras | own diagonal]
	int DC, DP;
	int64_t nc, np;
	std::vector<int64_t> ptr;
	std::vector<int32_t> brow;
	CLists lists;
	TStructure(int dc, int dp, int64_t n_cams, const CLists &r_lists)
		:DC(dc), DP(dp), nc(n_cams), np(int64_t(r_lists.size())), lists(r_lists)
	{
		for(int64_t c = 0; c < nc; ++ c) {
			ptr.push_back(int64_t(brow.size()));
			brow.push_back(int32_t(c));
		}
		for(int64_t pt = 0; pt < np; ++ pt) {
			ptr.push_back(int64_t(brow.size()));
			brow.insert(brow.end(), lists[pt].begin(), lists[pt].end());
			brow.push_back(int32_t(nc + pt));
		}
		ptr.push_back(int64_t(brow.size()));
	}
	SchurStructure Get() const { return SchurStructure{DC, DP, nc, np, ptr.data(), brow.data(), ptr[nc]}; }
};

struct TAnalysis { // what schur_analyze and schur_tiles_build have on the host
	SchurTileTables T;
	bool b_in_use = false;
	raw_vector<int32_t> obs_pt, obs_cam;
	std::vector<int64_t> sb_ptr;
	std::vector<int32_t> sb_row, sb_col;
	raw_vector<int32_t> ent_a;
	raw_vector<int64_t> ent_uoff;
	raw_vector<int64_t> run_rec;
	int64_t n_entries = 0;
	bool b_sorted_lists = false; // the comparison-sort branch (by size)
};

static void analyze(TAnalysis &A, const TStructure &r_st, int n_mode) // the order of schur_analyze
{
	const SchurStructure s = r_st.Get();
	for(int64_t pt = 0; pt < s.np; ++ pt) {
		for(int32_t n_cam : r_st.lists[pt]) {
			A.obs_pt.push_back(int32_t(pt));
			A.obs_cam.push_back(n_cam);
		}
		A.n_entries += s.n_K(pt) * (s.n_K(pt) + 1) / 2;
	}
	const int n_workers = host_thread_count(s.np, 65536);
	auto Tiles = [&]() {
		A.b_in_use = schur_tile_routes(A.T, n_mode, s);
		if(!A.b_in_use)
			return;
		A.run_rec.resize(A.T.p_runs->run_lm.size());
		schur_run_records(A.run_rec.data(), A.T.p_runs->run_lm.data(), int64_t(A.run_rec.size()), s);
		schur_tile_reduce_lists(A.T, s, A.sb_row, A.sb_col);
		schur_tile_xlists(A.T, s);
	};
	if(s.nc * s.nc <= (int64_t(1) << 26)) {
		schur_blocks_from_bitmap(A.sb_row, A.sb_col, s, A.obs_cam, n_workers);
		Tiles();
		if(!A.b_in_use)
			schur_lists_by_counting(A.sb_ptr, A.ent_a, A.ent_uoff, s, A.obs_cam, A.n_entries, A.sb_row.size(), n_workers);
	} else {
		A.b_sorted_lists = true;
		schur_lists_by_sorting(A.sb_ptr, A.sb_row, A.sb_col, A.ent_a, A.ent_uoff, s, A.obs_cam, A.obs_pt, A.n_entries);
		Tiles();
	}
}

// every table as bytes, for the comparisons between knobs
template <class V> static void put(std::string &r_s, const V &r_v) { r_s.append((const char*)r_v.data(), r_v.size() * sizeof(r_v[0])); r_s.push_back('|'); }
static std::string snapshot(const TAnalysis &A)
{
	std::string s;
	const SchurTileTables &T = A.T;
	s += std::string(T.p_s_keep_rule? T.p_s_keep_rule : "in use") + "|";
	put(s, A.sb_row); put(s, A.sb_col); put(s, A.sb_ptr); put(s, A.ent_a); put(s, A.ent_uoff);
	if(!A.b_in_use)
		return s;
	const int64_t counts[] = {T.n_all_pairs, T.n_run_points, T.n_prefix_points, T.n_tiles, T.n_slots, T.n_tile_points, T.n_list_points,
		T.n_tile_pairs, T.n_max_slots, T.n_max_k, T.n_rb};
	s.append((const char*)counts, sizeof(counts));
	s.append((const char*)T.n_run_jobs, sizeof(T.n_run_jobs));
	s.append((const char*)T.n_run_job_first, sizeof(T.n_run_job_first));
	for(const TRunJob &j : T.p_runs->jobs) {
		const int64_t f[] = {j.n_first, j.n_points, j.n_k, j.n_rb, j.n_cb, j.n_pad, j.n_pbase};
		s.append((const char*)f, sizeof(f));
	}
	put(s, T.p_runs->run_lm); put(s, T.p_runs->run_k); put(s, A.run_rec); put(s, T.slot_key);
	put(s, T.tile_ptr); put(s, T.tile_lm); put(s, T.tile_slot_ptr); put(s, T.pair_ptr); put(s, T.lm_slot);
	put(s, T.rb_ptr); put(s, T.rb_part); put(s, T.rb_sb);
	put(s, T.xpoints); put(s, T.xsb_ptr); put(s, T.xsb_map); put(s, T.xent_a); put(s, T.xent_uoff); put(s, T.xcam_ptr); put(s, T.xcam_obs);
	return s;
}

// ---- the checks ----

struct TEntry { int64_t key, a, b; bool operator ==(const TEntry &o) const { return key == o.key && a == o.a && b == o.b; } };

// the contribution lists of every block: (block, a, b) in block order, inside a block in (landmark, a, b) order
static void check_full_lists(const TStructure &r_st, const std::vector<int64_t> &sb_ptr, const std::vector<int32_t> &sb_row,
	const std::vector<int32_t> &sb_col, const raw_vector<int32_t> &ent_a, const raw_vector<int64_t> &ent_uoff)
{
	const SchurStructure s = r_st.Get();
	const int64_t ubase = s.n_ablocks * s.DC * s.DC, BLK = s.DC * s.DP, PP = s.DP * s.DP;
	std::vector<TEntry> want;
	for(int64_t pt = 0; pt < s.np; ++ pt) {
		const int64_t k = s.n_K(pt), o0 = s.n_First_Obs(pt);
		for(int64_t a = 0; a < k; ++ a)
			for(int64_t b = a; b < k; ++ b)
				want.push_back(TEntry{int64_t(r_st.lists[pt][a]) * s.nc + r_st.lists[pt][b], o0 + a, ubase + (o0 + b) * BLK + pt * PP});
	}
	std::stable_sort(want.begin(), want.end(), [](const TEntry &x, const TEntry &y) { return x.key < y.key; });
	CHECK(sb_ptr.size() == sb_row.size() + 1 && sb_row.size() == sb_col.size());
	CHECK(sb_ptr.front() == 0 && sb_ptr.back() == int64_t(want.size()));
	CHECK(ent_a.size() == want.size() && ent_uoff.size() == want.size());
	for(size_t i = 0; i < sb_row.size(); ++ i) {
		CHECK(sb_ptr[i] < sb_ptr[i + 1]);
		for(int64_t e = sb_ptr[i]; e < sb_ptr[i + 1]; ++ e)
			CHECK((want[e] == TEntry{int64_t(sb_col[i]) * s.nc + sb_row[i], ent_a[e], ent_uoff[e]}));
	}
}

static void check_block_list(const TStructure &r_st, const std::vector<int32_t> &sb_row, const std::vector<int32_t> &sb_col)
{
	std::set<int64_t> keys;
	for(const std::vector<int32_t> &r_list : r_st.lists)
		for(size_t a = 0; a < r_list.size(); ++ a)
			for(size_t b = a; b < r_list.size(); ++ b)
				keys.insert(int64_t(r_list[a]) * r_st.nc + r_list[b]);
	CHECK(sb_row.size() == keys.size() && sb_col.size() == keys.size());
	size_t i = 0;
	for(int64_t key : keys) {
		CHECK(int64_t(sb_col[i]) * r_st.nc + sb_row[i] == key);
		++ i;
	}
}

static int64_t piece_length(int64_t k_run, int DC)
{
	const int OB = 64 / DC;
	const int64_t n_mult = dev_knob_set("SLAMPP_HIP_DEV_RUN_PIECE_MULT")? std::max(1, std::min(4, dev_knob("SLAMPP_HIP_DEV_RUN_PIECE_MULT", 1))) : 1;
	return ((std::min<int64_t>(k_run, OB) * DC > 48)? 32 : 64) * n_mult;
}

// decodes the tables of an analysis that is in use; returns the branches it met.  p_pieces: the pieces' lengths, sorted
static std::set<std::string> check_tables(const TStructure &r_st, const TAnalysis &A, int n_mode, std::vector<int64_t> *p_pieces = 0)
{
	std::set<std::string> reached;
	const SchurStructure s = r_st.Get();
	const SchurTileTables &T = A.T;
	const CLists &L = r_st.lists;
	const int DC = s.DC, OB = 64 / DC;
	const int64_t nc = s.nc, np = s.np, ubase = s.n_ablocks * DC * DC, BLK = DC * s.DP, PP = s.DP * s.DP;
	const raw_vector<int32_t> &run_lm = T.p_runs->run_lm, &run_k = T.p_runs->run_k;
	const raw_vector<TRunJob> &jobs = T.p_runs->jobs;
	std::vector<std::vector<int> > delivered(np); // per landmark and pair b (b + 1) / 2 + a: deliveries to the right block
	int64_t n_all_pairs = 0;
	for(int64_t pt = 0; pt < np; ++ pt) {
		delivered[pt].assign(size_t(s.n_K(pt) * (s.n_K(pt) + 1) / 2), 0);
		n_all_pairs += s.n_K(pt) * (s.n_K(pt) + 1) / 2;
	}
	auto Key = [&](int64_t pt, int64_t a, int64_t b) { return int64_t(L[pt][a]) * nc + L[pt][b]; };
	// ---- routes ----
	std::vector<int> route(np, 0); // 1 run, 2 tile, 3 lists
	for(int32_t pt : run_lm) { CHECK(pt >= 0 && pt < np && !route[pt]); route[pt] = 1; }
	for(int32_t pt : T.tile_lm) { CHECK(pt >= 0 && pt < np && !route[pt]); route[pt] = 2; }
	for(int32_t pt : T.xpoints) { CHECK(pt >= 0 && pt < np && !route[pt]); route[pt] = 3; }
	int64_t n_pairs_taken = 0, n_prefix_points = 0;
	for(int64_t pt = 0; pt < np; ++ pt) {
		CHECK(route[pt] != 0);
		CHECK(T.handled[pt] == (route[pt] != 3));
		if(route[pt] != 3)
			n_pairs_taken += s.n_K(pt) * (s.n_K(pt) + 1) / 2;
		if(!s.n_K(pt))
			reached.insert("unobserved");
	}
	CHECK(T.n_run_points == int64_t(run_lm.size()) && T.n_tile_points == int64_t(T.tile_lm.size()) && T.n_list_points == int64_t(T.xpoints.size()));
	CHECK(T.n_all_pairs == n_all_pairs && T.n_tile_pairs == n_pairs_taken);
	CHECK(std::is_sorted(T.xpoints.begin(), T.xpoints.end()));
	CHECK(n_mode != 2 || run_lm.empty());
	CHECK(n_mode != 3 || T.tile_lm.empty());
	// ---- run jobs ----
	CHECK(run_k.size() == run_lm.size() && A.run_rec.size() == run_lm.size());
	for(size_t i = 0; i < run_lm.size(); ++ i) {
		CHECK(run_k[i] == s.n_K(run_lm[i]) && run_k[i] >= 1);
		CHECK(A.run_rec[i] == ubase + s.n_First_Obs(run_lm[i]) * BLK + run_lm[i] * PP); // the values hold [U .. U | C] per landmark
	}
	std::set<int64_t> piece_starts;
	for(const TRunJob &j : jobs)
		piece_starts.insert(j.n_first);
	std::map<int64_t, int64_t> piece_end;
	std::set<std::pair<int64_t, std::pair<int, int> > > piece_jobs; // (piece, rb, cb) met
	std::vector<int64_t> pieces;
	for(auto it = piece_starts.begin(); it != piece_starts.end(); ++ it) {
		auto it_next = std::next(it);
		const int64_t n_first = *it, n_end = (it_next == piece_starts.end())? int64_t(run_lm.size()) : *it_next;
		CHECK(n_first >= 0 && n_first < n_end);
		CHECK(it != piece_starts.begin() || n_first == 0); // (every landmark of the run list is in a piece)
		piece_end[n_first] = n_end;
		pieces.push_back(n_end - n_first);
		const int32_t pt0 = run_lm[n_first];
		CHECK(n_end - n_first <= piece_length(s.n_K(pt0), DC));
		if(piece_length(s.n_K(pt0), DC) < piece_length(1, DC))
			reached.insert("pieces_of_32");
		bool b_prefix_piece = false;
		for(int64_t m = n_first; m < n_end; ++ m) { // every member's list is a prefix of the first member's, lengths do not increase
			const int32_t pt = run_lm[m];
			CHECK(m == n_first || run_k[m] <= run_k[m - 1]);
			CHECK(std::equal(L[pt].begin(), L[pt].end(), L[pt0].begin()));
			b_prefix_piece = b_prefix_piece || run_k[m] < run_k[n_first];
		}
		if(b_prefix_piece)
			reached.insert("prefix_runs");
		// (n_prefix_points counts the members of chains of several classes; a lower bound from the tables: members of pieces with a shorter member)
		n_prefix_points += b_prefix_piece? n_end - n_first : 0;
	}
	CHECK(T.n_prefix_points >= n_prefix_points && T.n_prefix_points <= T.n_run_points);
	CHECK(dev_knob_set("SLAMPP_HIP_DEV_NO_PREFIX_RUNS")? T.n_prefix_points == 0 : true);
	std::sort(pieces.begin(), pieces.end());
	if(p_pieces)
		*p_pieces = pieces;
	if(!jobs.empty())
		reached.insert("runs");
	int64_t n_jobs_seen = 0;
	std::vector<int> slot_owner(size_t(T.n_slots), 0); // partial blocks: written by exactly one job or tile
	CHECK(int64_t(T.slot_key.size()) == T.n_slots);
	for(int nt = 0; nt < 5; ++ nt) {
		for(int d = 0; d < 2; ++ d) {
			bool b_any_flag = false;
			for(int x = 0; x < 2; ++ x) {
				CHECK(nt >= 1 || !T.n_run_jobs[nt][d][x]);
				CHECK(T.n_run_job_first[nt][d][x] >= 0 && T.n_run_job_first[nt][d][x] + T.n_run_jobs[nt][d][x] <= int64_t(jobs.size()));
				n_jobs_seen += T.n_run_jobs[nt][d][x];
				for(int64_t ji = 0; ji < T.n_run_jobs[nt][d][x]; ++ ji) {
					const TRunJob &j = jobs[T.n_run_job_first[nt][d][x] + ji];
					const int64_t n_end = piece_end.at(j.n_first), k = j.n_k, rb = j.n_rb, cb = j.n_cb;
					const int32_t pt0 = run_lm[j.n_first];
					CHECK(k == s.n_K(pt0) && j.n_pad == 0);
					CHECK(cb >= 0 && cb <= rb && rb * OB < k);
					CHECK(piece_jobs.insert(std::make_pair(int64_t(j.n_first), std::make_pair(int(rb), int(cb)))).second);
					const int64_t n_kb_r = std::min<int64_t>(OB, k - rb * OB), n_kb_c = std::min<int64_t>(OB, k - cb * OB);
					CHECK(nt == (int(std::max(n_kb_r, n_kb_c)) * DC + 15) / 16 && d == int(rb == cb));
					int64_t n_reach = 0; // members with observations in row block rb: the first ones
					while(j.n_first + n_reach < n_end && run_k[j.n_first + n_reach] > rb * OB)
						++ n_reach;
					CHECK(j.n_points == n_reach && n_reach >= 1);
					const bool b_flag = run_k[j.n_first + n_reach - 1] < k;
					b_any_flag = b_any_flag || b_flag;
					CHECK(!b_flag || x == 1); // (a job without the flag is in the masking launch when another of its class has it: below)
					if(rb > 0)
						reached.insert("second_observation_block");
					int64_t n_slot = j.n_pbase;
					for(int64_t ob = 0; ob < n_kb_r; ++ ob) { // the order the kernel numbers its partial blocks in
						for(int64_t oa = 0; oa < ((rb == cb)? ob + 1 : n_kb_c); ++ oa, ++ n_slot) {
							const int64_t a = cb * OB + oa, b = rb * OB + ob;
							CHECK(n_slot >= 0 && n_slot < T.n_run_slots && !slot_owner[n_slot]);
							slot_owner[n_slot] = 1;
							CHECK(T.slot_key[n_slot] == Key(pt0, a, b));
							for(int64_t m = 0; m < j.n_points; ++ m) { // a landmark reads as zero beyond its own last observation
								if(b < run_k[j.n_first + m])
									++ delivered[run_lm[j.n_first + m]][b * (b + 1) / 2 + a];
							}
						}
					}
				}
			}
			// folded into the masking launch exactly when one of the class's jobs has the flag
			CHECK(b_any_flag? T.n_run_jobs[nt][d][0] == 0 : T.n_run_jobs[nt][d][1] == 0);
			if(b_any_flag)
				reached.insert("masking_launch");
		}
	}
	CHECK(n_jobs_seen == int64_t(jobs.size()));
	for(int64_t pc : piece_starts) { // every pair of observation blocks of every piece has its job
		const int64_t n_blocks = (s.n_K(run_lm[pc]) + OB - 1) / OB;
		for(int rb = 0; rb < n_blocks; ++ rb)
			for(int cb = 0; cb <= rb; ++ cb)
				CHECK(piece_jobs.count(std::make_pair(pc, std::make_pair(rb, cb))));
	}
	// ---- tiles ----
	const int n_max_points = std::max(1, dev_knob("SLAMPP_HIP_DEV_TILE_POINTS", int(SCHUR_TILE_MAX_POINTS)));
	CHECK(int64_t(T.tile_ptr.size()) == T.n_tiles + 1 && int64_t(T.tile_slot_ptr.size()) == T.n_tiles + 1 && int64_t(T.pair_ptr.size()) == np + 1);
	CHECK(T.tile_ptr[0] == 0 && T.tile_ptr.back() == int64_t(T.tile_lm.size()) && T.tile_slot_ptr[0] == T.n_run_slots && T.tile_slot_ptr.back() == T.n_slots);
	int64_t n_max_slots = 0, n_max_k = 0;
	for(int64_t t = 0; t < T.n_tiles; ++ t) {
		const int64_t n_slots = T.tile_slot_ptr[t + 1] - T.tile_slot_ptr[t], n_points = T.tile_ptr[t + 1] - T.tile_ptr[t];
		CHECK(n_slots >= 0 && n_slots <= SCHUR_TILE_SLOTS && n_points >= 1 && n_points <= n_max_points);
		n_max_slots = std::max(n_max_slots, n_slots);
		if(n_slots == SCHUR_TILE_SLOTS && t + 1 < T.n_tiles)
			reached.insert("tile_closed_at_64_blocks");
		if(n_points == SCHUR_TILE_MAX_POINTS && t + 1 < T.n_tiles)
			reached.insert("tile_closed_at_64_points");
		int64_t n_pairs = 0;
		for(int64_t i = T.tile_ptr[t]; i < T.tile_ptr[t + 1]; ++ i) {
			const int64_t pt = T.tile_lm[i], k = s.n_K(pt);
			CHECK(k <= tile_max_k(SCHUR_TILE_SLOTS));
			n_max_k = std::max(n_max_k, k);
			CHECK(T.pair_ptr[pt] >= 0 && T.pair_ptr[pt] + k * (k + 1) / 2 <= int64_t(T.lm_slot.size()));
			for(int64_t b = 0; b < k; ++ b) {
				for(int64_t a = 0; a <= b; ++ a, ++ n_pairs) {
					const int64_t n_slot = T.lm_slot[T.pair_ptr[pt] + b * (b + 1) / 2 + a];
					CHECK(n_slot < n_slots && T.slot_key[T.tile_slot_ptr[t] + n_slot] == Key(pt, a, b));
					slot_owner[T.tile_slot_ptr[t] + n_slot] = 2;
					++ delivered[pt][b * (b + 1) / 2 + a];
				}
			}
		}
		CHECK(n_mode > 0 || n_pairs >= 3 * n_slots); // (the library decides: a kept tile's landmarks share their blocks)
	}
	if(T.n_tiles) {
		reached.insert("tiles");
		CHECK(T.n_max_slots == n_max_slots && T.n_max_k == n_max_k);
		const int n_loads = tile_launch_loads(DC, s.DP, T.n_max_k);
		CHECK(n_loads >= 1 && n_loads <= 4);
		if(nc > 65536)
			reached.insert("tile_order_from_lists");
	}
	for(int64_t g = 0; g < T.n_slots; ++ g)
		CHECK(slot_owner[g] != 0);
	// ---- reduce lists ----
	CHECK(T.n_rb == int64_t(T.rb_sb.size()) && int64_t(T.rb_ptr.size()) == T.n_rb + 1 && int64_t(T.rb_part.size()) == T.n_slots);
	CHECK(T.rb_ptr[0] == 0 && T.rb_ptr.back() == T.n_slots);
	std::vector<int> in_list(size_t(T.n_slots), 0);
	for(int64_t i = 0; i < T.n_rb; ++ i) {
		CHECK(T.rb_ptr[i] < T.rb_ptr[i + 1]); // blocks without partials are absent
		CHECK(i == 0 || T.rb_sb[i - 1] < T.rb_sb[i]);
		CHECK(T.rb_sb[i] >= 0 && size_t(T.rb_sb[i]) < A.sb_row.size());
		const int64_t key = int64_t(A.sb_col[T.rb_sb[i]]) * nc + A.sb_row[T.rb_sb[i]];
		for(int64_t e = T.rb_ptr[i]; e < T.rb_ptr[i + 1]; ++ e) {
			const int32_t g = T.rb_part[e];
			CHECK(g >= 0 && g < T.n_slots && !in_list[g] ++);
			CHECK(e == T.rb_ptr[i] || T.rb_part[e - 1] < g);
			CHECK(T.slot_key[g] == key);
		}
	}
	if(nc * nc > (int64_t(1) << 24))
		reached.insert("block_of_by_bisection");
	// ---- x-lists ----
	if(T.n_list_points > 0) {
		reached.insert("xlists");
		CHECK(T.xsb_ptr.size() == T.xsb_map.size() + 1 && T.xsb_ptr[0] == 0 && T.xsb_ptr.back() == int64_t(T.xent_a.size()) && T.xent_a.size() == T.xent_uoff.size());
		for(size_t i = 0; i < T.xsb_map.size(); ++ i) {
			CHECK(T.xsb_ptr[i] < T.xsb_ptr[i + 1] && (i == 0 || T.xsb_map[i - 1] < T.xsb_map[i]));
			const int64_t key = int64_t(A.sb_col[T.xsb_map[i]]) * nc + A.sb_row[T.xsb_map[i]];
			int64_t n_prev[3] = {-1, -1, -1};
			for(int64_t e = T.xsb_ptr[i]; e < T.xsb_ptr[i + 1]; ++ e) {
				CHECK(T.xent_a[e] >= 0 && size_t(T.xent_a[e]) < A.obs_pt.size());
				const int64_t pt = A.obs_pt[T.xent_a[e]], o0 = s.n_First_Obs(pt), a = T.xent_a[e] - o0, k = s.n_K(pt);
				CHECK(route[pt] == 3);
				const int64_t n_rel = T.xent_uoff[e] - ubase - pt * PP - o0 * BLK;
				CHECK(n_rel >= 0 && n_rel % BLK == 0);
				const int64_t b = n_rel / BLK;
				CHECK(a >= 0 && a <= b && b < k && Key(pt, a, b) == key);
				const int64_t n_cur[3] = {pt, a, b};
				CHECK(std::lexicographical_compare(n_prev, n_prev + 3, n_cur, n_cur + 3)); // (landmark, a, b) order
				std::copy(n_cur, n_cur + 3, n_prev);
				++ delivered[pt][b * (b + 1) / 2 + a];
			}
		}
		std::vector<std::vector<int32_t> > cam_obs(nc); // the leftover landmarks' observations per camera, in landmark order
		for(int32_t pt : T.xpoints) {
			if(s.n_K(pt) > tile_max_k(SCHUR_TILE_SLOTS))
				reached.insert("over_tile_max_k");
			if(s.n_K(pt) > OB)
				reached.insert("long_track_on_lists");
			for(int64_t a = 0; a < s.n_K(pt); ++ a)
				cam_obs[L[pt][a]].push_back(int32_t(s.n_First_Obs(pt) + a));
		}
		CHECK(int64_t(T.xcam_ptr.size()) == nc + 1 && T.xcam_ptr[0] == 0 && T.xcam_ptr[nc] == int64_t(T.xcam_obs.size()));
		for(int64_t c = 0; c < nc; ++ c) {
			CHECK(T.xcam_ptr[c + 1] - T.xcam_ptr[c] == int64_t(cam_obs[c].size()));
			CHECK(std::equal(cam_obs[c].begin(), cam_obs[c].end(), T.xcam_obs.begin() + T.xcam_ptr[c]));
		}
	} else
		CHECK(T.xent_a.empty() && T.xpoints.empty());
	// ---- coverage: every (landmark, a <= b) delivered exactly once, to its block ----
	for(int64_t pt = 0; pt < np; ++ pt)
		for(int n_times : delivered[pt])
			CHECK(n_times == 1);
	return reached;
}

// ---- the cases ----

static std::vector<int32_t> cams(int n_first, int n_count)
{
	std::vector<int32_t> v;
	for(int i = 0; i < n_count; ++ i)
		v.push_back(n_first + i);
	return v;
}
static void add(CLists &r_lists, int n_times, const std::vector<int32_t> &r_list) { r_lists.insert(r_lists.end(), size_t(n_times), r_list); }

struct TKnobs { // development knobs of a scope (with SLAMPP_HIP_DEV=1)
	std::vector<std::string> names;
	TKnobs(std::initializer_list<std::pair<const char*, const char*> > knobs)
	{
		setenv("SLAMPP_HIP_DEV", "1", 1);
		for(const auto &r_knob : knobs) {
			setenv(r_knob.first, r_knob.second, 1);
			names.push_back(r_knob.first);
		}
		dev_knobs_refresh();
	}
	~TKnobs()
	{
		for(const std::string &r_name : names)
			unsetenv(r_name.c_str());
		unsetenv("SLAMPP_HIP_DEV");
		dev_knobs_refresh();
	}
};

static int n_failed = 0;

static void print_case(const std::string &r_name, std::set<std::string> reached)
{
	printf("%s: reached", r_name.c_str());
	for(const std::string &r_tag : reached)
		printf(" %s", r_tag.c_str());
	printf(" ok\n");
	fflush(stdout);
}

// runs the builders on the structure, checks everything, and prints the case's line; returns the bytes of the tables
static std::string run_case(const std::string &r_name, const TStructure &r_st, int n_mode, bool b_print = true,
	std::function<void(const TAnalysis&, const std::vector<int64_t>&)> extra = nullptr)
{
	try {
		TAnalysis A;
		analyze(A, r_st, n_mode);
		std::set<std::string> reached;
		std::vector<int64_t> pieces;
		if(A.b_in_use)
			reached = check_tables(r_st, A, n_mode, &pieces);
		else {
			CHECK(A.T.p_s_keep_rule || n_mode == 0);
			reached.insert(std::string("rule_") + (A.T.p_s_keep_rule? A.T.p_s_keep_rule : "off"));
			for(int nt = 0; nt < 5; ++ nt)
				for(int d = 0; d < 2; ++ d)
					for(int x = 0; x < 2; ++ x)
						CHECK(!A.T.n_run_jobs[nt][d][x] && !A.T.n_run_job_first[nt][d][x]);
		}
		if(A.b_sorted_lists) {
			reached.insert("comparison_sort_lists");
			check_block_list(r_st, A.sb_row, A.sb_col);
			check_full_lists(r_st, A.sb_ptr, A.sb_row, A.sb_col, A.ent_a, A.ent_uoff);
		} else {
			check_block_list(r_st, A.sb_row, A.sb_col); // from the bitmap
			if(!A.b_in_use) {
				reached.insert("counting_sort_lists");
				check_full_lists(r_st, A.sb_ptr, A.sb_row, A.sb_col, A.ent_a, A.ent_uoff);
			}
		}
		if(r_st.np >= (int64_t(1) << 18) || dev_knob_set("SLAMPP_HIP_DEV_RUN_HASH_ONLY"))
			reached.insert("hashes_alone");
		if(host_thread_count(r_st.np, 65536) > 1)
			reached.insert("many_workers");
		if(extra)
			extra(A, pieces);
		if(b_print)
			print_case(r_name, reached);
		return snapshot(A);
	} catch(std::exception &r_exc) {
		printf("%s: FAILED %s\n", r_name.c_str(), r_exc.what());
		fflush(stdout);
		++ n_failed;
		return "failed " + r_name;
	}
}

// both full-list branches on one small structure, whatever the sizes would choose
static void both_list_sorts(const TStructure &r_st)
{
	const SchurStructure s = r_st.Get();
	raw_vector<int32_t> obs_pt, obs_cam;
	int64_t n_entries = 0;
	for(int64_t pt = 0; pt < s.np; ++ pt) {
		for(int32_t n_cam : r_st.lists[pt]) {
			obs_pt.push_back(int32_t(pt));
			obs_cam.push_back(n_cam);
		}
		n_entries += s.n_K(pt) * (s.n_K(pt) + 1) / 2;
	}
	for(int n_workers : {1, 3}) {
		std::vector<int64_t> sb_ptr[2];
		std::vector<int32_t> sb_row[2], sb_col[2];
		raw_vector<int32_t> ent_a[2];
		raw_vector<int64_t> ent_uoff[2];
		schur_blocks_from_bitmap(sb_row[0], sb_col[0], s, obs_cam, n_workers);
		schur_lists_by_counting(sb_ptr[0], ent_a[0], ent_uoff[0], s, obs_cam, n_entries, sb_row[0].size(), n_workers);
		schur_lists_by_sorting(sb_ptr[1], sb_row[1], sb_col[1], ent_a[1], ent_uoff[1], s, obs_cam, obs_pt, n_entries);
		for(int i = 0; i < 2; ++ i) {
			check_block_list(r_st, sb_row[i], sb_col[i]);
			check_full_lists(r_st, sb_ptr[i], sb_row[i], sb_col[i], ent_a[i], ent_uoff[i]);
		}
	}
}

// runs, chains, tile landmarks, a long lone track and a landmark nobody sees, n_copies times on cameras of their own
static CLists mixed_lists(int n_copies, int n_cams_per_copy /* >= 60 */)
{
	CLists lists;
	for(int c = 0; c < n_copies; ++ c) {
		const int o = c * n_cams_per_copy;
		add(lists, 5, cams(o, 3));                          // a run
		add(lists, 3, cams(o + 4, 8)); add(lists, 3, cams(o + 4, 6)); // a chain inside the first observation block
		add(lists, 2, cams(o + 14, 13)); add(lists, 2, cams(o + 14, 11)); add(lists, 2, cams(o + 14, 10)); // one that ends in the second
		for(int j = 1; j <= 3; ++ j)
			add(lists, 3, {o + 30, o + 30 + j});               // landmarks that share a tile (runs where two are enough)
		add(lists, 1, cams(o + 40, 12));                    // a lone long track
		add(lists, 1, {});                                  // nobody sees it
	}
	return lists;
}

static void expect_same(const char *p_s_what, const std::string &r_a, const std::string &r_b)
{
	if(r_a != r_b) {
		printf("%s: FAILED the tables differ\n", p_s_what);
		++ n_failed;
	}
}

static void thread_cases()
{
	const TStructure st(6, 3, 40 * 60, mixed_lists(40, 60));
	std::string s_plain = run_case("mixed-40-plain", st, -1, false), s_grain, s_one, s_hash;
	{
		TKnobs knobs({{"SLAMPP_HIP_DEV_HOST_THREAD_GRAIN", "256"}, {"SLAMPP_HIP_DEV_EMIT_THREADS", "8"}});
		s_grain = run_case("mixed-40-many-workers", st, -1);
		both_list_sorts(st);
	}
	{
		TKnobs knobs({{"SLAMPP_HIP_DEV_HOST_THREAD_GRAIN", "256"}, {"SLAMPP_HIP_DEV_EMIT_THREADS", "1"}});
		s_one = run_case("mixed-40-one-emitter", st, -1, false);
	}
	{
		TKnobs knobs({{"SLAMPP_HIP_DEV_HOST_THREAD_GRAIN", "256"}, {"SLAMPP_HIP_DEV_RUN_HASH_ONLY", "1"}});
		s_hash = run_case("mixed-40-hashes-alone", st, -1);
	}
	expect_same("thread grain 256 against unset", s_grain, s_plain);
	expect_same("emitting threads 1 against 8", s_one, s_grain);
	expect_same("hashes alone against list comparison", s_hash, s_plain);
	{
		TKnobs knobs({{"SLAMPP_HIP_DEV_HOST_THREAD_GRAIN", "256"}, {"SLAMPP_HIP_DEV_NO_PREFIX_RUNS", "1"}});
		run_case("mixed-40-no-prefix-runs", st, -1);
	}
	{
		TKnobs knobs({{"SLAMPP_HIP_DEV_HOST_THREAD_GRAIN", "256"}});
		CLists lists;
		std::mt19937 rng(7);
		for(int i = 0; i < 5000; ++ i) {
			std::set<int32_t> c;
			while(c.size() < 3)
				c.insert(int32_t(rng() % 200));
			lists.push_back(std::vector<int32_t>(c.begin(), c.end()));
		}
		run_case("random-many-workers", TStructure(6, 3, 200, lists), -1); // (the counting sort of all contributions on many workers)
	}
}

static void small_cases()
{
	{ // identical-list runs of 4, 64, 65 and 129 landmarks; 33 of nine cameras (pieces of 32)
		CLists lists;
		add(lists, 4, cams(0, 3)); add(lists, 64, cams(3, 3)); add(lists, 65, cams(6, 3)); add(lists, 129, cams(9, 3)); add(lists, 33, cams(12, 9));
		const TStructure st(6, 3, 40, lists);
		run_case("runs-4-64-65-129", st, -1, true, [](const TAnalysis&, const std::vector<int64_t> &r_pieces) {
			CHECK((r_pieces == std::vector<int64_t>{1, 1, 1, 4, 32, 64, 64, 64, 64})); });
		TKnobs knobs({{"SLAMPP_HIP_DEV_RUN_PIECE_MULT", "2"}});
		run_case("runs-piece-mult-2", st, -1, true, [](const TAnalysis&, const std::vector<int64_t> &r_pieces) {
			CHECK((r_pieces == std::vector<int64_t>{1, 4, 33, 64, 65, 128})); }); // (129 = 128 + 1; 33 of nine cameras: one piece of up to 64)
	}
	{ // prefix chains ending inside the first observation block (OB = 10), at its boundary, and in the second block
		CLists lists;
		add(lists, 5, cams(0, 8)); add(lists, 3, cams(0, 6));
		add(lists, 3, cams(40, 10)); add(lists, 2, cams(40, 9));
		add(lists, 3, cams(20, 13)); add(lists, 2, cams(20, 11)); add(lists, 2, cams(20, 10));
		run_case("prefix-chains", TStructure(6, 3, 60, lists), -1, true, [](const TAnalysis &A, const std::vector<int64_t> &r_pieces) {
			CHECK((r_pieces == std::vector<int64_t>{5, 7, 8}) && A.T.n_prefix_points == 20); });
	}
	{ // two long tracks (k > OB) alone are a run; a lone one lands on the lists
		CLists lists;
		add(lists, 2, cams(0, 12)); add(lists, 1, cams(20, 12));
		run_case("long-tracks", TStructure(6, 3, 40, lists), -1, true, [](const TAnalysis &A, const std::vector<int64_t>&) {
			CHECK(A.T.n_run_points == 2 && A.T.n_list_points == 1); });
	}
	{ // a tile closed at exactly 64 blocks and a landmark that would make it 65; 64 landmarks in a tile and a 65th; k = 11; k = 0
		CLists lists;
		add(lists, 1, {0, 1, 2});                 // six blocks
		for(int j = 3; j <= 31; ++ j)
			add(lists, 1, {0, j});                 // two more each: 64
		add(lists, 1, {32});                      // one more block
		add(lists, 65, {40, 41});
		add(lists, 1, cams(50, 11));
		add(lists, 1, {});
		run_case("tile-limits", TStructure(6, 3, 64, lists), 2, true, [](const TAnalysis &A, const std::vector<int64_t>&) {
			CHECK(A.T.n_max_slots == 64 && A.T.n_list_points == 1 && A.T.n_max_k == 3); });
	}
	const int shapes[3][2] = {{6, 3}, {7, 3}, {3, 2}};
	for(int n_mode : {-1, 1, 2, 3}) { // every mode at every block shape
		for(const int (&shape)[2] : shapes) {
			const TStructure st(shape[0], shape[1], 120, mixed_lists(2, 60));
			run_case("mixed-mode" + std::to_string(n_mode) + "-" + std::to_string(shape[0]) + "x" + std::to_string(shape[1]), st, n_mode);
			if(n_mode == -1)
				both_list_sorts(st);
		}
	}
	{ // equal lengths, all lists distinct and sharing nothing: no run is possible, no tile is kept
		CLists lists;
		for(int i = 0; i < 20; ++ i)
			add(lists, 1, {2 * i, 2 * i + 1});
		run_case("rule-runs-impossible", TStructure(6, 3, 40, lists), -1);
		for(int i = 0; i < 5; ++ i)
			add(lists, 1, cams(40 + 3 * i, 3));
		run_case("rule-no-jobs", TStructure(6, 3, 60, lists), -1);
		add(lists, 4, {56, 57});
		run_case("rule-under-half", TStructure(6, 3, 60, lists), -1);
		run_case("mode-0", TStructure(6, 3, 60, lists), 0);
	}
}

static void large_cases()
{
	std::mt19937 rng(11);
	{ // 65 536 leftover landmarks with random cameras: the sample says the lists keep them
		CLists lists;
		for(int i = 0; i < 65536 + 64; ++ i) {
			std::set<int32_t> c;
			while(c.size() < 3)
				c.insert(int32_t(rng() % 300));
			lists.push_back(std::vector<int32_t>(c.begin(), c.end()));
		}
		run_case("rule-sample", TStructure(6, 3, 300, lists), -1);
	}
	{ // just over 2^18 landmarks in a few large classes: the hashes alone, and the check of every class against its lists
		CLists lists;
		for(int c = 0; c < 4; ++ c)
			add(lists, (1 << 16) + 2, {3 * c, 3 * c + 1});
		run_case("hashes-alone-by-size", TStructure(6, 3, 12, lists), -1);
	}
	for(int64_t nc : {70000, 8200, 4100}) { // cameras beyond the 16-bit sort fields; the comparison-sort lists; Block_Of by bisection behind the bitmap
		CLists lists;
		for(int i = 0; i < 300; ++ i) {
			std::set<int32_t> c;
			const int32_t n_first = int32_t(rng() % 16) * int32_t(nc / 16);
			while(c.size() < size_t(2 + i % 3))
				c.insert(n_first + int32_t(rng() % 6));
			lists.push_back(std::vector<int32_t>(c.begin(), c.end()));
		}
		add(lists, 5, {int32_t(nc - 3), int32_t(nc - 1)});
		add(lists, 1, cams(int(nc - 30), 12));
		run_case("cameras-" + std::to_string(nc), TStructure(6, 3, nc, lists), 1);
	}
}

int main(int n_arg_num, char **p_arg_list)
{
	const bool b_threads_only = n_arg_num > 1 && !strcmp(p_arg_list[1], "threads");
	thread_cases();
	if(!b_threads_only) {
		small_cases();
		large_cases();
	}
	return n_failed != 0;
}
