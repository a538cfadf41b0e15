// schur_tile_tables.cpp -- host tables of the reduced camera system's assembly (schur_tile_tables.h): the landmarks with the
// same cameras (runs), the others sorted by their first two cameras and cut into tiles, the partial blocks of every block
// of S, the lists of the landmarks neither takes, and the contribution lists of every block.  One function per job; the
// three steps at the end of the tile part run them in the analysis' order.
#include "schur_tile_tables.h"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>

namespace slampp {

void SchurTileTables::Phase(const char *p_s_name)
{
	if(!b_timing)
		return;
	const double t = wall_ms();
	fprintf(stderr, "[schur tiles] %-20s %8.2f ms\n", p_s_name, t - t_phase);
	t_phase = t;
}

size_t SchurTileTables::n_Block_Of(int64_t n_key) const
{
	if(!key_sb.empty())
		return (key_sb[size_t(n_key)] >= 0)? size_t(key_sb[size_t(n_key)]) : sb_keys.size();
	const size_t k = size_t(std::lower_bound(sb_keys.begin(), sb_keys.end(), n_key) - sb_keys.begin());
	return (k < sb_keys.size() && sb_keys[k] == n_key)? k : sb_keys.size();
}

namespace {

// ---------------------------------------------------------------------------------------------
// shared by the passes
// ---------------------------------------------------------------------------------------------

// (the passes over the landmarks that do not depend on each other run on a few threads: at C5's two million landmarks
// telling the classes apart was 98 ms of a 250 ms analysis on one core, a cache miss per list)
template <class CWork>
void for_landmark_ranges(int64_t n_begin, int64_t np, CWork work)
{
	for_ranges(n_begin, np, host_thread_count(np - n_begin, 65536), [&](int, int64_t n_first, int64_t n_last) { work(n_first, n_last); });
}

// LSD radix sort of items by bits [n_first_bit, n_last_bit) of their 64-bit keys, 11 bits a pass (2 048 destinations a thread:
// the writes of a pass stay in the caches; with 16-bit digits every write was a miss), stable, on up to eight threads: a thread
// counts the digits of its range, the ranges' counts are laid out digit by digit and thread by thread -- where a serial pass
// would have put the elements --, and every thread moves its own range.  The items carry what later passes need: nothing is
// read through the permutation.
template <class TItem, class CKeyOf>
void radix_sort_items(raw_vector<TItem> &r_items, raw_vector<TItem> &r_tmp, int n_first_bit, int n_last_bit, CKeyOf key_of)
{
	enum { DIGIT_BITS = 11, DIGITS = 1 << DIGIT_BITS };
	const int64_t n = int64_t(r_items.size());
	r_tmp.resize(size_t(n));
	const int n_workers = host_thread_count(n, 32768);
	std::vector<std::vector<int64_t> > cnt(n_workers, std::vector<int64_t>(DIGITS));
	for(int n_shift = n_first_bit; n_shift < n_last_bit; n_shift += DIGIT_BITS) {
		const uint64_t n_mask = (n_last_bit - n_shift >= DIGIT_BITS)? uint64_t(DIGITS - 1) : (uint64_t(1) << (n_last_bit - n_shift)) - 1;
		for_ranges(0, n, n_workers, [&](int t, int64_t n_first, int64_t n_last) {
			std::vector<int64_t> &r_cnt = cnt[t];
			std::fill(r_cnt.begin(), r_cnt.end(), 0);
			for(int64_t i = n_first; i < n_last; ++ i)
				++ r_cnt[(key_of(r_items[i]) >> n_shift) & n_mask];
		});
		int64_t n_sum = 0;
		for(int d = 0; d < DIGITS; ++ d) {
			for(int t = 0; t < n_workers; ++ t) {
				const int64_t n_here = cnt[t][d];
				cnt[t][d] = n_sum;
				n_sum += n_here;
			}
		}
		for_ranges(0, n, n_workers, [&](int t, int64_t n_first, int64_t n_last) {
			std::vector<int64_t> &r_cnt = cnt[t];
			for(int64_t i = n_first; i < n_last; ++ i)
				r_tmp[r_cnt[(key_of(r_items[i]) >> n_shift) & n_mask] ++] = r_items[i];
		});
		r_items.swap(r_tmp);
	}
}

bool same_list(const SchurStructure &s, int32_t p, int32_t q)
{
	const int64_t k = s.n_K(p);
	return s.n_K(q) == k && std::equal(s.p_Cams(p), s.p_Cams(p) + k, s.p_Cams(q));
}

bool list_less(const SchurStructure &s, int32_t p, int32_t q) // lexicographic: a list sorts right before its continuations
{
	return std::lexicographical_compare(s.p_Cams(p), s.p_Cams(p) + s.n_K(p), s.p_Cams(q), s.p_Cams(q) + s.n_K(q));
}

bool is_prefix(const SchurStructure &s, int32_t p, int32_t q) // the list of p starts the list of q
{
	const int64_t kp = s.n_K(p);
	return kp <= s.n_K(q) && std::equal(s.p_Cams(p), s.p_Cams(p) + kp, s.p_Cams(q));
}

// the one way out on which the contribution lists keep everything (SLAMPP_HIP_PLAN_TIMING: the machine-readable report
// beside the "[schur] of N landmarks" line; diagnostics only)
bool keep_lists(SchurTileTables &T, const char *p_s_rule)
{
	T.p_s_keep_rule = p_s_rule;
	memset(T.n_run_jobs, 0, sizeof(T.n_run_jobs));
	memset(T.n_run_job_first, 0, sizeof(T.n_run_job_first));
	if(T.b_timing)
		fprintf(stderr, "[schur report] the lists keep everything: rule=%s\n", p_s_rule);
	return false;
}

template <class CCounts>
void report_counts(const CCounts &r_counts, const char *p_s_end = "\n") // "value x times, ..." of a histogram
{
	const char *p_s_sep = "";
	for(const auto &r_count : r_counts) {
		fprintf(stderr, "%s%lldx%lld", p_s_sep, (long long)r_count.first, (long long)r_count.second);
		p_s_sep = ",";
	}
	fprintf(stderr, "%s%s", r_counts.empty()? "-" : "", p_s_end);
}

// ---------------------------------------------------------------------------------------------
// runs: landmarks with identical camera lists, found by sorting hashes of the lists
// ---------------------------------------------------------------------------------------------

// what the comparison of neighbours needs of a landmark -- both hashes, the length of its list -- travels with it through
// the sort (24 bytes an element, read in order, instead of reads of hash[], hash2[] and k_of[] in the order of the pass
// before: a cache miss each, 12 + 8 ms at C5's two million landmarks)
struct TSortItem { uint64_t n_hash, n_hash2; int32_t n_k, n_landmark; };
struct TClass { int64_t n_first, n_count; }; // landmarks order[n_first .. n_first + n_count): seen by the same cameras
struct TGroup { size_t c0, c1; int64_t n_members; }; // a run: classes [c0, c1), every list continuing the one before it

struct TRunWork { // what the passes over the runs hand each other
	raw_vector<uint64_t> hash, hash2; // (hash2: a second, independent hash of the same list -- mark_same_lists; raw_vector: not zero-filled, host_pool.h)
	raw_vector<int32_t> k_of;         // observations per landmark (8 MB that stay in the caches better than two reads of ptr[] per use)
	raw_vector<TSortItem> items, items_tmp;
	raw_vector<int32_t> order;        // the landmarks by hash
	raw_vector<uint8_t> same_as_previous; // order[i] is seen by the cameras of order[i - 1]
	std::vector<TClass> classes;
	// what the chains ask of every class: the length of its list, the tiles of its job, whether it continues the class before it
	raw_vector<int32_t> class_k;
	raw_vector<uint8_t> class_tiles, class_continues;
	std::vector<TGroup> groups;
	int64_t n_emit_members = 0;
};

void hash_lists(TRunWork &W, const SchurStructure &s)
{
	W.hash.resize(size_t(s.np));
	W.hash2.resize(size_t(s.np));
	W.k_of.resize(size_t(s.np));
	for_landmark_ranges(0, s.np, [&](int64_t n_first, int64_t n_last) {
		for(int64_t pt = n_first; pt < n_last; ++ pt) {
			const int64_t k = s.n_K(pt);
			const int32_t *p_cam = s.p_Cams(pt);
			W.k_of[pt] = int32_t(k);
			uint64_t h = 0x9E3779B97F4A7C15ull * uint64_t(k + 1), h2 = 0xCBF29CE484222325ull ^ uint64_t(k);
			for(int64_t i = 0; i < k; ++ i) {
				h ^= uint64_t(p_cam[i]) + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
				h *= 0xFF51AFD7ED558CCDull;
				h2 = (h2 ^ (uint64_t(p_cam[i]) + 0x632BE59BD9B4E019ull * uint64_t(i + 1))) * 0x100000001B3ull;
				h2 ^= h2 >> 29;
			}
			W.hash[pt] = h;
			W.hash2[pt] = h2;
		}
	});
}

// Radix sort by the hash (radix_sort_items): equal hashes stay in landmark order.
void sort_by_hash(TRunWork &W, const SchurStructure &s)
{
	W.items.resize(size_t(s.np));
	W.items_tmp.resize(size_t(s.np));
	W.order.resize(size_t(s.np));
	for_landmark_ranges(0, s.np, [&](int64_t n_first, int64_t n_last) {
		for(int64_t pt = n_first; pt < n_last; ++ pt) {
			TSortItem &r_item = W.items[pt];
			r_item.n_hash = W.hash[pt];
			r_item.n_hash2 = W.hash2[pt];
			r_item.n_k = W.k_of[pt];
			r_item.n_landmark = int32_t(pt);
		}
	});
	// (by the upper 33 bits: three passes.  Lists whose hashes differ only below -- a few hundred pairs among two million --
	// may come out interleaved; the classes are then cut where mark_same_lists says so, and the chains put classes of
	// one list back together: the same runs)
	radix_sort_items(W.items, W.items_tmp, 31, 64, [](const TSortItem &r_item) { return r_item.n_hash; });
}

// Two neighbours of the sorted order have the same cameras if both 64-bit hashes and the lengths agree: 128 bits over at
// most a few million lists (two different lists agreeing in both: below 1e-25 an analysis).  Reading the two lists
// themselves -- four dependent cache misses per landmark, in hash order -- was 20 ms of C5's analysis on eight threads;
// systems under 262 144 landmarks (where it costs nothing) still do (SLAMPP_HIP_DEV_RUN_HASH_ONLY, a development knob:
// the hashes alone there too, for the tests).
void mark_same_lists(TRunWork &W, const SchurStructure &s)
{
	const int64_t np = s.np;
	W.same_as_previous.resize(size_t(np));
	W.same_as_previous[0] = 0;
	W.order[0] = W.items[0].n_landmark;
	const bool b_compare_lists = np < (int64_t(1) << 18) && !dev_knob_set("SLAMPP_HIP_DEV_RUN_HASH_ONLY");
	for_landmark_ranges(1, np, [&](int64_t n_first, int64_t n_last) {
		for(int64_t i = n_first; i < n_last; ++ i) {
			const TSortItem &r_p = W.items[i - 1], &r_q = W.items[i];
			W.order[i] = r_q.n_landmark;
			W.same_as_previous[i] = r_q.n_hash == r_p.n_hash && r_q.n_hash2 == r_p.n_hash2 && r_q.n_k == r_p.n_k &&
				(!b_compare_lists || same_list(s, r_p.n_landmark, r_q.n_landmark));
		}
	});
	if(b_compare_lists)
		return;
	// the hashes alone said "same": every class of more than one landmark is held to its lists once, first member
	// against last (two lists per class instead of two per landmark: two unkeyed hashes of the same 32-bit indices are
	// not 128 independent bits).  A mismatch -- never seen -- sends every neighbour through same_list().
	std::atomic<int> n_collisions(0);
	for_landmark_ranges(1, np, [&](int64_t n_first, int64_t n_last) {
		for(int64_t i = n_first; i < n_last; ++ i) {
			if(W.same_as_previous[i] && (i + 1 == np || !W.same_as_previous[i + 1])) { // the last member of a class
				int64_t f = i;
				while(f > 0 && W.same_as_previous[f])
					-- f; // (may leave this thread's range: read only)
				if(!same_list(s, W.items[f].n_landmark, W.items[i].n_landmark))
					n_collisions.fetch_add(1, std::memory_order_relaxed);
			}
		}
	});
	if(n_collisions.load()) {
		for_landmark_ranges(1, np, [&](int64_t n_first, int64_t n_last) {
			for(int64_t i = n_first; i < n_last; ++ i)
				W.same_as_previous[i] = W.same_as_previous[i] && same_list(s, W.items[i - 1].n_landmark, W.items[i].n_landmark);
		});
	}
}

// what the emission asks of a run whose longest list has k_longest cameras (a lone long track is no better off in a run
// than in the lists; two of them already share their partial blocks)
inline int64_t min_run_members(int64_t k_longest, int64_t n_min_run, int OB)
{
	return (k_longest > OB && n_min_run > 2)? 2 : n_min_run;
}

// Every list as long as every other: then no list continues another, a run is a class of landmarks with the same cameras,
// and if the largest class is too small to be one there is no run anywhere -- the classes need not be formed, ordered and
// walked to find that out (the uniform-visibility C4, three pairs of equal lists among half a million, spent 28 ms
// of its 57 ms analysis ordering half a million classes of one landmark each).  The largest class = the longest stretch of
// "same as previous" + 1: per range of the sorted order, then over the ranges' ends.
bool runs_impossible(const TRunWork &W, int64_t np, int64_t n_min_run, int OB)
{
	if(n_min_run < 2 || np <= 1)
		return false;
	struct TStretch { int64_t n_first, n_last, n_head, n_tail, n_longest; int32_t k_min, k_max; }; // head / tail: stretches at the range's ends
	std::vector<TStretch> parts;
	std::mutex t_mutex;
	for_landmark_ranges(0, np, [&](int64_t n_first, int64_t n_last) {
		TStretch t = {n_first, n_last, 0, 0, 0, INT32_MAX, 0};
		int64_t n_current = 0;
		bool b_head = true;
		for(int64_t i = n_first; i < n_last; ++ i) {
			if(W.same_as_previous[i])
				++ n_current;
			else {
				if(b_head)
					t.n_head = n_current;
				b_head = false;
				t.n_longest = std::max(t.n_longest, n_current);
				n_current = 0;
			}
			t.k_min = std::min(t.k_min, int32_t(W.items[i].n_k));
			t.k_max = std::max(t.k_max, int32_t(W.items[i].n_k));
		}
		if(b_head)
			t.n_head = n_current; // (the whole range is one stretch)
		t.n_tail = n_current;
		t.n_longest = std::max(t.n_longest, n_current);
		std::lock_guard<std::mutex> t_lock(t_mutex);
		parts.push_back(t);
	});
	std::sort(parts.begin(), parts.end(), [](const TStretch &a, const TStretch &b) { return a.n_first < b.n_first; });
	int64_t n_longest = 0, n_open = 0; // (n_open: the stretch that reaches the end of the ranges seen so far)
	int32_t k_min = INT32_MAX, k_max = 0;
	for(const TStretch &t : parts) {
		const bool b_whole = t.n_head == t.n_last - t.n_first; // every entry of the range continues a stretch
		n_longest = std::max(n_longest, std::max(t.n_longest, n_open + t.n_head));
		n_open = b_whole? n_open + t.n_head : t.n_tail;
		k_min = std::min(k_min, t.k_min);
		k_max = std::max(k_max, t.k_max);
	}
	return k_min == k_max && n_longest + 1 < min_run_members(k_max, n_min_run, OB);
}

void form_classes(TRunWork &W, const SchurStructure &s)
{
	for(int64_t i = 0; i < s.np;) {
		int64_t j = i + 1;
		while(j < s.np && W.same_as_previous[j])
			++ j;
		if(s.n_K(W.order[i]) >= 1)
			W.classes.push_back(TClass{i, j - i});
		i = j;
	}
}

// The classes in the order of their lists, a list right before its continuations: by a 64-bit key of the first cameras of
// the list (a radix sort on a few threads), the lists themselves only where keys tie -- a comparison sort that reads two
// lists per comparison was 96 ms at 500 000 landmarks with 500 000 different lists (uniform visibility).  Camera + 1 in
// every field, zero behind the end of a short list: the keys order the first fields' worth of cameras the way list_less does.
void order_classes_by_key(TRunWork &W, const SchurStructure &s)
{
	const int64_t n_classes = int64_t(W.classes.size());
	int n_field_bits = 1;
	while((int64_t(1) << n_field_bits) <= s.nc)
		++ n_field_bits;
	const int n_fields = std::max(1, 64 / n_field_bits), n_key_bits = n_fields * n_field_bits;
	struct TClassItem { uint64_t n_key; TClass t_class; };
	raw_vector<TClassItem> class_items(n_classes), class_items_tmp;
	for_ranges(0, n_classes, host_thread_count(n_classes, 16384), [&](int, int64_t n_first, int64_t n_last) {
		for(int64_t c = n_first; c < n_last; ++ c) {
			const int32_t p = W.order[W.classes[c].n_first];
			const int64_t k = s.n_K(p);
			const int32_t *p_cam = s.p_Cams(p);
			uint64_t n_key = 0;
			for(int f = 0; f < n_fields; ++ f)
				n_key = (n_key << n_field_bits) | ((f < k)? uint64_t(p_cam[f]) + 1 : 0);
			class_items[c].n_key = n_key;
			class_items[c].t_class = W.classes[c];
		}
	});
	radix_sort_items(class_items, class_items_tmp, 0, n_key_bits, [](const TClassItem &r_item) { return r_item.n_key; }); // (stable: classes of one key stay in the order they were found in)
	std::vector<TClass> sorted(W.classes.size());
	for(int64_t c = 0; c < n_classes; ++ c)
		sorted[c] = class_items[c].t_class;
	for(int64_t c0 = 0; c0 < n_classes;) { // keys that tie: lists longer than the key that agree in all of its fields
		int64_t c1 = c0 + 1;
		while(c1 < n_classes && class_items[c1].n_key == class_items[c0].n_key)
			++ c1;
		if(c1 - c0 > 1) {
			std::sort(sorted.begin() + c0, sorted.begin() + c1, [&](const TClass &a, const TClass &b) {
				const int32_t p = W.order[a.n_first], q = W.order[b.n_first];
				return list_less(s, p, q) || (!list_less(s, q, p) && a.n_first < b.n_first); });
		}
		c0 = c1;
	}
	W.classes.swap(sorted);
}

// read from the lists on a few threads (500 000 classes of one landmark each, uniform visibility, were 15 ms of cache
// misses in the loop of group_chains)
void read_class_lists(TRunWork &W, const SchurStructure &s, int OB, bool b_chains)
{
	const int64_t n_classes = int64_t(W.classes.size());
	W.class_k.resize(size_t(n_classes));
	W.class_tiles.resize(size_t(n_classes));
	W.class_continues.resize(size_t(n_classes));
	for_ranges(0, n_classes, host_thread_count(n_classes, 16384), [&](int, int64_t n_first, int64_t n_last) {
		for(int64_t c = n_first; c < n_last; ++ c) {
			const int32_t p = W.order[W.classes[c].n_first];
			const int64_t k = s.n_K(p);
			W.class_k[c] = int32_t(k);
			W.class_tiles[c] = uint8_t((std::min<int64_t>(k, OB) * s.DC + 15) / 16); // 16-line tiles a side of the landmark's (first) job
			W.class_continues[c] = b_chains && c > 0 && is_prefix(s, W.order[W.classes[c - 1].n_first], p);
		}
	});
}

// A run is a CHAIN of classes -- landmarks seen by exactly the same cameras -- in which every class's camera list continues
// the one before it (tracks born at the same camera and lost at different ones; identical lists are the special case).  A
// landmark reads as zero beyond its own last observation (run_k), so the chain's partial blocks are those of its longest
// list, written once per piece of 64 landmarks instead of once per class: at the Venice-like C4 the classes of the long
// tracks have 2 - 17 members and 66 - 465 blocks of S each.  Chains of short lists break where the matrix-core tiles of a
// job would grow (16 lines a tile): a landmark of two cameras does not pay for ten.
void group_chains(TRunWork &W, int64_t n_min_run, int OB)
{
	const std::vector<TClass> &classes = W.classes;
	for(size_t c0 = 0; c0 < classes.size();) {
		size_t c1 = c0 + 1;
		int64_t n_members = classes[c0].n_count;
		while(c1 < classes.size() && W.class_tiles[c1] == W.class_tiles[c0] && W.class_continues[c1]) {
			n_members += classes[c1].n_count;
			++ c1;
		}
		if(n_members >= min_run_members(W.class_k[c1 - 1], n_min_run, OB)) {
			W.groups.push_back(TGroup{c0, c1, n_members});
			W.n_emit_members += n_members;
		}
		c0 = c1;
	}
}

// what a pass over runs leaves behind (the runs are emitted by a few threads, each into one of these, and the results put
// behind each other in the runs' order -- the tables come out as one thread wrote them)
struct TEmitOut {
	raw_vector<int32_t> run_lm, run_k;
	raw_vector<int64_t> slot_key;
	std::vector<TRunJob> jobs_nt[5][2][2];
	int64_t n_run_pairs = 0, n_prefix_points = 0;
	std::vector<int32_t> members, members_k; // (scratch)
};

struct CRunEmitter {
	const SchurStructure &s;
	const TRunWork &W;
	int OB;
	int64_t n_piece_max, n_piece_mult;
	bool b_piece_knob;

	// Longer pieces (a job takes its landmarks 64 at a time and keeps its sums across those sub-pieces) leave half or a
	// quarter of the partial blocks behind -- and were measured no faster (Venice-like C4 1.491 / 1.519 / 1.569 ms
	// at 1 / 2 / 4 times the base length: the longest jobs set the length of a launch; C5 1.197 / 1.223 / 1.183): the
	// kernel can, the analysis does not ask for it (development knob, tests/test_schur_gpu.py)
	CRunEmitter(const SchurStructure &r_s, const TRunWork &r_work)
		:s(r_s), W(r_work), OB(64 / r_s.DC), n_piece_max(std::max(1, std::min(64, dev_knob("SLAMPP_HIP_DEV_RUN_PIECE", 64)))),
		n_piece_mult(dev_knob_set("SLAMPP_HIP_DEV_RUN_PIECE_MULT")? std::max(1, std::min(4, dev_knob("SLAMPP_HIP_DEV_RUN_PIECE_MULT", 1))) : 1),
		b_piece_knob(dev_knob_set("SLAMPP_HIP_DEV_RUN_PIECE"))
	{}

	// the jobs of one run: the members (landmarks), longest camera list first -- every other member's list is that
	// list or a prefix of it; pieces of at most 64 landmarks, a job per pair of observation blocks, over the piece's
	// landmarks that reach into the row block (they are the first ones: sorted by length).  p_members_k null: every
	// member has k_all observations.  Positions and offsets in the jobs are relative to r_out until the merge.
	void Emit_Run(TEmitOut &r_out, const int32_t *p_members, const int32_t *p_members_k, int64_t n_members, int64_t k_all) const
	{
		raw_vector<int32_t> &run_lm = r_out.run_lm, &run_k = r_out.run_k;
		raw_vector<int64_t> &slot_key = r_out.slot_key;
		const int DC = s.DC;
		const int64_t nc = s.nc;
		// (pieces of 32 where a job keeps ten or sixteen accumulator tiles -- nine cameras and up at 6 x 6 --: those jobs are
		// the long ones, and more of them spread better: 164 + 123 -> 130 + 103 us for the two widest kernels of the
		// Venice-like C4, for 18 us more in the reduction of the partial blocks)
		const int64_t k_run = p_members_k? p_members_k[0] : k_all;
		const int64_t n_piece_len = ((std::min<int64_t>(k_run, OB) * DC > 48 && !b_piece_knob)? 32 : n_piece_max) * n_piece_mult;
		for(int64_t f = 0; f < n_members; f += n_piece_len) {
			const int64_t n_piece = std::min<int64_t>(n_piece_len, n_members - f);
			const int32_t pt0 = p_members[f];
			const int64_t k = s.n_K(pt0); // the piece's longest list
			const int32_t *p_cam = s.p_Cams(pt0);
			const int64_t n_blocks = (k + OB - 1) / OB;
			const int64_t n_lm_first = int64_t(run_lm.size());
			// (the landmarks' lengths come with the members, class by class, and `handled` is set in a pass of its own:
			// a read of k_of[] and a write of handled[] per landmark, both in hash order, were most of the 20 ms this loop took
			// at C5's two million landmarks)
			run_lm.insert(run_lm.end(), p_members + f, p_members + f + n_piece);
			if(p_members_k) {
				run_k.insert(run_k.end(), p_members_k + f, p_members_k + f + n_piece);
				for(int64_t e = f; e < f + n_piece; ++ e)
					r_out.n_run_pairs += int64_t(p_members_k[e]) * (p_members_k[e] + 1) / 2;
			} else { // (one class: the same list for all of them -- no copy of the members, no array of equal lengths)
				run_k.insert(run_k.end(), size_t(n_piece), int32_t(k_all));
				r_out.n_run_pairs += n_piece * (k_all * (k_all + 1) / 2);
			}
			for(int64_t rb = 0; rb < n_blocks; ++ rb) {
				const int64_t n_kb_r = std::min<int64_t>(OB, k - rb * OB);
				int64_t n_reach = p_members_k? 0 : n_piece; // landmarks of the piece with observations in row block rb (one class: all of them)
				while(n_reach < n_piece && run_k[size_t(n_lm_first + n_reach)] > rb * OB)
					++ n_reach;
				for(int64_t cb = 0; cb <= rb; ++ cb) {
					const int64_t n_kb_c = std::min<int64_t>(OB, k - cb * OB);
					TRunJob job;
					job.n_first = int32_t(n_lm_first);
					job.n_points = int32_t(n_reach);
					job.n_k = int32_t(k);
					job.n_rb = int32_t(rb);
					job.n_cb = int32_t(cb);
					job.n_pad = 0;
					job.n_pbase = int64_t(slot_key.size());
					for(int64_t ob = 0; ob < n_kb_r; ++ ob) { // the order the kernel numbers its partial blocks in
						for(int64_t oa = 0; oa < ((rb == cb)? ob + 1 : n_kb_c); ++ oa)
							slot_key.push_back(int64_t(p_cam[cb * OB + oa]) * nc + p_cam[rb * OB + ob]);
					}
					const int n_lines = int(std::max(n_kb_r, n_kb_c)) * DC;
					const bool b_job_prefix = run_k[size_t(n_lm_first + n_reach - 1)] < k; // (sorted: the last one is the shortest)
					r_out.jobs_nt[(n_lines + 15) / 16][rb == cb][b_job_prefix].push_back(job);
				}
			}
		}
	}

	void Emit_Groups(TEmitOut &r_out, size_t g0, size_t g1) const
	{
		for(size_t g = g0; g < g1; ++ g) {
			const size_t c0 = W.groups[g].c0, c1 = W.groups[g].c1;
			const int64_t n_members = W.groups[g].n_members, k_longest = W.class_k[c1 - 1];
			if(c1 - c0 == 1)
				Emit_Run(r_out, W.order.data() + W.classes[c0].n_first, 0, n_members, k_longest); // (the members as they lie in the sorted order)
			else {
				r_out.members.clear();
				r_out.members_k.clear();
				for(size_t c = c1; c > c0; -- c) { // longest list first
					const TClass &r_class = W.classes[c - 1];
					r_out.members.insert(r_out.members.end(), W.order.begin() + r_class.n_first, W.order.begin() + r_class.n_first + r_class.n_count);
					r_out.members_k.insert(r_out.members_k.end(), size_t(r_class.n_count), W.class_k[c - 1]);
				}
				Emit_Run(r_out, r_out.members.data(), r_out.members_k.data(), int64_t(r_out.members.size()), 0);
				r_out.n_prefix_points += n_members;
			}
		}
	}
};

// the emitting threads' outputs behind each other, in the order of the runs: positions in the run list and offsets of the
// partial blocks become global
void merge_emit_outputs(SchurTileTables &T, std::vector<TEmitOut> &r_outs, std::vector<TRunJob> (&jobs_nt)[5][2][2])
{
	raw_vector<int32_t> &run_lm = T.p_runs->run_lm, &run_k = T.p_runs->run_k;
	if(r_outs.size() == 1) {
		run_lm.swap(r_outs[0].run_lm);
		run_k.swap(r_outs[0].run_k);
		T.slot_key.swap(r_outs[0].slot_key);
		for(int nt = 0; nt < 5; ++ nt)
			for(int d = 0; d < 2; ++ d)
				for(int x = 0; x < 2; ++ x)
					jobs_nt[nt][d][x].swap(r_outs[0].jobs_nt[nt][d][x]);
	} else {
		for(TEmitOut &r_out : r_outs) {
			const int64_t n_lm_base = int64_t(run_lm.size()), n_slot_base = int64_t(T.slot_key.size());
			for(int nt = 0; nt < 5; ++ nt) {
				for(int d = 0; d < 2; ++ d) {
					for(int x = 0; x < 2; ++ x) {
						for(TRunJob &r_job : r_out.jobs_nt[nt][d][x]) {
							r_job.n_first = int32_t(r_job.n_first + n_lm_base);
							r_job.n_pbase += n_slot_base;
						}
						jobs_nt[nt][d][x].insert(jobs_nt[nt][d][x].end(), r_out.jobs_nt[nt][d][x].begin(), r_out.jobs_nt[nt][d][x].end());
					}
				}
			}
			run_lm.insert(run_lm.end(), r_out.run_lm.begin(), r_out.run_lm.end());
			run_k.insert(run_k.end(), r_out.run_k.begin(), r_out.run_k.end());
			T.slot_key.insert(T.slot_key.end(), r_out.slot_key.begin(), r_out.slot_key.end());
		}
	}
	for(const TEmitOut &r_out : r_outs) {
		T.n_run_pairs += r_out.n_run_pairs;
		T.n_prefix_points += r_out.n_prefix_points;
	}
}

// the runs on a few threads, ranges of groups with about the same number of landmarks; each thread marks the landmarks of
// its runs in T.handled (a landmark is in one run: no two threads write the same byte)
void emit_runs(SchurTileTables &T, const TRunWork &W, const SchurStructure &s, std::vector<TRunJob> (&jobs_nt)[5][2][2])
{
	const CRunEmitter emitter(s, W);
	const std::vector<TGroup> &groups = W.groups;
	const int64_t n_emit_members = W.n_emit_members;
	const int n_emit_workers = host_thread_count(n_emit_members, 65536, dev_knob("SLAMPP_HIP_DEV_EMIT_THREADS", 8)); // (development aid, plan.h: 1 = one thread, for comparing the tables)
	std::vector<TEmitOut> outs;
	outs.resize(size_t(n_emit_workers));
	std::vector<size_t> g_begin(size_t(n_emit_workers) + 1, groups.size());
	g_begin[0] = 0;
	int64_t n_seen = 0;
	int n_next = 1;
	for(size_t g = 0; g < groups.size() && n_next < n_emit_workers; ++ g) {
		n_seen += groups[g].n_members;
		while(n_next < n_emit_workers && n_seen >= n_emit_members * n_next / n_emit_workers)
			g_begin[size_t(n_next ++)] = g + 1;
	}
	run_on_threads(n_emit_workers, [&](int t) {
		outs[size_t(t)].run_lm.reserve(size_t(n_emit_members / n_emit_workers + 65536));
		outs[size_t(t)].run_k.reserve(size_t(n_emit_members / n_emit_workers + 65536));
		emitter.Emit_Groups(outs[size_t(t)], g_begin[size_t(t)], g_begin[size_t(t) + 1]);
		for(int32_t n_landmark : outs[size_t(t)].run_lm)
			T.handled[size_t(n_landmark)] = 1;
	});
	merge_emit_outputs(T, outs, jobs_nt);
}

// one launch per (tiles a side, diagonal): where some jobs of a class have landmarks that end early, all its jobs
// run the masking instance (its masks do nothing for the others; ten launches of a few thousand waves each, one
// after the other, cost more in ragged ends than the masks do)
void fold_run_jobs(SchurTileTables &T, std::vector<TRunJob> (&jobs_nt)[5][2][2])
{
	raw_vector<TRunJob> &jobs = T.p_runs->jobs;
	for(int nt = 1; nt <= 4; ++ nt) {
		for(int d = 0; d < 2; ++ d) {
			if(!jobs_nt[nt][d][1].empty()) {
				jobs_nt[nt][d][1].insert(jobs_nt[nt][d][1].end(), jobs_nt[nt][d][0].begin(), jobs_nt[nt][d][0].end());
				jobs_nt[nt][d][0].clear();
			}
			for(int x = 0; x < 2; ++ x) {
				T.n_run_job_first[nt][d][x] = int64_t(jobs.size());
				T.n_run_jobs[nt][d][x] = int64_t(jobs_nt[nt][d][x].size());
				jobs.insert(jobs.end(), jobs_nt[nt][d][x].begin(), jobs_nt[nt][d][x].end());
			}
		}
	}
}

// the passes above in order; returns whether every list is as long as every other and no class large enough for a run
// (for the report)
bool find_runs(SchurTileTables &T, const SchurStructure &s, int64_t n_min_run)
{
	const int OB = 64 / s.DC;
	TRunWork W;
	hash_lists(W, s);
	T.Phase("hashes");
	sort_by_hash(W, s);
	T.Phase("sort");
	mark_same_lists(W, s);
	T.Phase("  same lists");
	const bool b_runs_impossible = runs_impossible(W, s.np, n_min_run, OB);
	T.p_runs->run_lm.reserve(b_runs_impossible? 0 : s.np);
	T.p_runs->run_k.reserve(b_runs_impossible? 0 : s.np);
	if(!b_runs_impossible)
		form_classes(W, s);
	T.Phase("  classes");
	const bool b_chains = !dev_knob_set("SLAMPP_HIP_DEV_NO_PREFIX_RUNS");
	if(b_chains)
		order_classes_by_key(W, s);
	T.Phase("  class order");
	read_class_lists(W, s, OB, b_chains);
	T.Phase("  class lists");
	group_chains(W, n_min_run, OB);
	std::vector<TRunJob> jobs_nt[5][2][2];
	emit_runs(T, W, s, jobs_nt);
	T.Phase("  emit (jobs)"); // (with the marks of the landmarks that are in runs: each emitting thread sets its own)
	fold_run_jobs(T, jobs_nt);
	Discard_Later(T.trash, W.hash); Discard_Later(T.trash, W.hash2); Discard_Later(T.trash, W.k_of); Discard_Later(T.trash, W.items);
	Discard_Later(T.trash, W.items_tmp); Discard_Later(T.trash, W.order); Discard_Later(T.trash, W.same_as_previous);
	return b_runs_impossible;
}

// ---------------------------------------------------------------------------------------------
// tiles: the other landmarks by (first camera, second camera) -- two counting sorts --, cut where a tile is full
// ---------------------------------------------------------------------------------------------

// the two cameras a landmark is sorted by travel with it -- (first camera, second camera, landmark) in one 64-bit word, two
// counting passes over the words: passes that read ptr[] and brow[] of every landmark in the order of the pass before were
// four cache misses a landmark and 23 ms at 500 000 landmarks.  nc <= 65536.
std::vector<int32_t> tile_order_by_fields(const SchurTileTables &T, const SchurStructure &s)
{
	raw_vector<uint64_t> items, items_tmp;
	items.reserve(size_t(s.np - T.n_run_points));
	for(int64_t pt = 0; pt < s.np; ++ pt) {
		if(T.handled[pt])
			continue;
		const int64_t k = s.n_K(pt);
		const uint64_t n_first_cam = (k == 0)? 0 : uint64_t(s.p_Cams(pt)[0]), n_second_cam = (k > 1)? uint64_t(s.p_Cams(pt)[1]) : n_first_cam;
		items.push_back((n_first_cam << 48) | (n_second_cam << 32) | uint64_t(pt));
	}
	const int64_t n_items = int64_t(items.size());
	items_tmp.resize(size_t(n_items));
	std::vector<int64_t> cnt(65537);
	for(int n_shift = 32; n_shift <= 48; n_shift += 16) { // least significant first
		std::fill(cnt.begin(), cnt.end(), 0);
		for(int64_t i = 0; i < n_items; ++ i)
			++ cnt[((items[i] >> n_shift) & 0xFFFF) + 1];
		for(int64_t c = 0; c < 65536; ++ c)
			cnt[c + 1] += cnt[c];
		for(int64_t i = 0; i < n_items; ++ i)
			items_tmp[cnt[(items[i] >> n_shift) & 0xFFFF] ++] = items[i];
		items.swap(items_tmp);
	}
	std::vector<int32_t> order(size_t(n_items), 0);
	for(int64_t i = 0; i < n_items; ++ i)
		order[i] = int32_t(uint32_t(items[i]));
	return order;
}

// cameras that do not fit the 16-bit fields: the passes read the lists
std::vector<int32_t> tile_order_by_lists(const SchurTileTables &T, const SchurStructure &s)
{
	std::vector<int32_t> order, tmp;
	for(int64_t pt = 0; pt < s.np; ++ pt) {
		if(!T.handled[pt])
			order.push_back(int32_t(pt));
	}
	tmp.resize(order.size());
	std::vector<int64_t> cnt(s.nc + 1);
	for(int n_pass = 0; n_pass < 2; ++ n_pass) {
		std::fill(cnt.begin(), cnt.end(), 0);
		auto Cam = [&](int64_t pt) -> int64_t {
			const int64_t k = s.n_K(pt);
			return (k == 0)? 0 : s.p_Cams(pt)[(n_pass == 0 && k > 1)? 1 : 0]; // least significant first
		};
		for(size_t i = 0; i < order.size(); ++ i)
			++ cnt[Cam(order[i]) + 1];
		for(int64_t c = 0; c < s.nc; ++ c)
			cnt[c + 1] += cnt[c];
		for(size_t i = 0; i < order.size(); ++ i)
			tmp[cnt[Cam(order[i])] ++] = order[i];
		order.swap(tmp);
	}
	return order;
}

// the tile under construction: its blocks of S by key, in a small open-addressed table
struct TSlotTable {
	enum { SIZE = 256 }; // > 2 * SCHUR_TILE_SLOTS
	int64_t keys[SIZE];
	int16_t slots[SIZE];
	int used[SIZE];
	int n_used;
	TSlotTable() :n_used(0) { for(int i = 0; i < SIZE; ++ i) slots[i] = -1; }
	static size_t n_Hash(int64_t key) { return size_t((uint64_t(key) * 0x9E3779B97F4A7C15ull) >> 56) & (SIZE - 1); }
	int n_Find(int64_t key) const
	{
		for(size_t h = n_Hash(key);; h = (h + 1) & (SIZE - 1)) {
			if(slots[h] < 0)
				return -1;
			if(keys[h] == key)
				return slots[h];
		}
	}
	void Insert(int64_t key, int n_slot)
	{
		size_t h = n_Hash(key);
		while(slots[h] >= 0)
			h = (h + 1) & (SIZE - 1);
		keys[h] = key;
		slots[h] = int16_t(n_slot);
		used[n_used ++] = int(h);
	}
	void Clear()
	{
		for(int i = 0; i < n_used; ++ i)
			slots[used[i]] = -1;
		n_used = 0;
	}
};

// the tile cutter: landmarks p_order[n_first .. n_last) in order, a tile closed where the next landmark would take it over
// SCHUR_TILE_SLOTS blocks or the point limit; a closed tile is kept if the library was told to (n_mode > 0) or its
// landmarks share enough (three contributions per block)
void build_run(TTileRun &R, const int32_t *p_order, int64_t n_first, int64_t n_last, int n_mode, const SchurStructure &s)
{
	const int n_cap = SCHUR_TILE_SLOTS, n_max_k = tile_max_k(SCHUR_TILE_SLOTS);
	const int n_max_points = std::max(1, dev_knob("SLAMPP_HIP_DEV_TILE_POINTS", int(SCHUR_TILE_MAX_POINTS)));
	TSlotTable table;
	std::vector<int32_t> cur_lm;
	std::vector<int64_t> cur_keys;
	std::vector<uint8_t> cur_slots;
	int64_t n_cur_pairs = 0;
	auto Close = [&]() {
		if(cur_lm.empty())
			return;
		const bool b_good = n_mode > 0 || n_cur_pairs >= 3 * int64_t(cur_keys.size());
		if(b_good) {
			R.tile_size.push_back(int32_t(cur_lm.size()));
			R.tile_lm.insert(R.tile_lm.end(), cur_lm.begin(), cur_lm.end());
			R.tile_slots.push_back(int32_t(cur_keys.size()));
			R.slot_key.insert(R.slot_key.end(), cur_keys.begin(), cur_keys.end());
			R.lm_slot.insert(R.lm_slot.end(), cur_slots.begin(), cur_slots.end());
		} else
			R.rejected.insert(R.rejected.end(), cur_lm.begin(), cur_lm.end());
		cur_lm.clear();
		cur_keys.clear();
		cur_slots.clear();
		n_cur_pairs = 0;
		table.Clear();
	};
	int64_t keys[SCHUR_TILE_SLOTS];
	for(int64_t i = n_first; i < n_last; ++ i) {
		const int32_t pt = p_order[i];
		const int64_t k = s.n_K(pt);
		const int32_t *p_cam = s.p_Cams(pt);
		if(k > n_max_k) {
			R.rejected.push_back(pt);
			continue;
		}
		const int n_pairs = int(k * (k + 1) / 2);
		int n_new = 0;
		for(int64_t b = 0, j = 0; b < k; ++ b) {
			for(int64_t a = 0; a <= b; ++ a, ++ j) {
				keys[j] = int64_t(p_cam[a]) * s.nc + p_cam[b]; // column = the smaller camera, row = the larger
				n_new += table.n_Find(keys[j]) < 0;
			}
		}
		if(int(cur_keys.size()) + n_new > n_cap || int(cur_lm.size()) >= n_max_points)
			Close();
		for(int j = 0; j < n_pairs; ++ j) {
			int n_slot = table.n_Find(keys[j]);
			if(n_slot < 0) {
				n_slot = int(cur_keys.size());
				table.Insert(keys[j], n_slot);
				cur_keys.push_back(keys[j]);
			}
			cur_slots.push_back(uint8_t(n_slot));
		}
		cur_lm.push_back(pt);
		n_cur_pairs += n_pairs;
	}
	Close();
}

// Where the library decides by itself and the runs alone do not carry half of the contributions, the tiles are tried on a
// sample first -- the first 4 096 landmarks of every piece -- and left alone if runs and tiles together would stay well
// under that half (under 30 %: the decision of schur_tile_routes asks for 50): landmarks that share no cameras with their
// neighbours in this order (uniform visibility) end up on the lists whatever the tiles find, and forming tiles of all
// 500 000 of them to learn that was 16 - 23 ms of the analysis.
bool sample_says_lists(const SchurTileTables &T, const std::vector<int32_t> &r_order, int n_pieces, int n_mode, const SchurStructure &s)
{
	const int64_t n_sample = 4096;
	std::vector<TTileRun> sample(n_pieces);
	std::vector<int64_t> sample_pairs(n_pieces, 0);
	for_ranges(0, int64_t(r_order.size()), n_pieces, [&](int t, int64_t n_first, int64_t n_piece_end) {
		const int64_t n_last = std::min(n_first + n_sample, n_piece_end);
		build_run(sample[t], r_order.data(), n_first, n_last, n_mode, s);
		for(int64_t i = n_first; i < n_last; ++ i) {
			const int64_t k = s.n_K(r_order[i]);
			sample_pairs[t] += k * (k + 1) / 2;
		}
	});
	int64_t n_sample_all = 0, n_sample_tiled = 0;
	for(int t = 0; t < n_pieces; ++ t) {
		n_sample_all += sample_pairs[t];
		n_sample_tiled += int64_t(sample[t].lm_slot.size());
	}
	// pairs outside the runs, and the share of them the sample says tiles would take
	const int64_t n_rest_pairs = T.n_all_pairs - T.n_run_pairs;
	const double f_tiled = n_sample_all? double(n_sample_tiled) / double(n_sample_all) : 0.0;
	if(T.b_timing)
		fprintf(stderr, "[schur tiles] sample: tiles take %.1f %% of the contributions outside the runs\n", 100 * f_tiled);
	return double(T.n_run_pairs) + f_tiled * double(n_rest_pairs) < 0.30 * double(T.n_all_pairs);
}

// orders the landmarks outside the runs and cuts them into tiles; false: the sample rule left everything to the lists
bool find_tiles(SchurTileTables &T, int n_mode, const SchurStructure &s)
{
	const std::vector<int32_t> order = (s.nc > 65536)? tile_order_by_lists(T, s) : tile_order_by_fields(T, s);
	const int64_t n_rest = int64_t(order.size());
	// built piecewise by a few threads (a piece boundary is a tile boundary: the pieces are counted from the landmarks
	// alone, not by host_thread_count() -- the tiles must not depend on the machine or on a knob)
	const int n_pieces = int(std::max<int64_t>(1, std::min<int64_t>(8, n_rest / 32768)));
	if(n_mode < 0 && n_rest >= 65536 && 2 * T.n_run_pairs < T.n_all_pairs && sample_says_lists(T, order, n_pieces, n_mode, s))
		return false;
	T.tile_pieces.resize(n_pieces);
	for_ranges(0, n_rest, n_pieces, [&](int t, int64_t n_first, int64_t n_last) {
		build_run(T.tile_pieces[t], order.data(), n_first, n_last, n_mode, s);
	});
	for(const TTileRun &R : T.tile_pieces) {
		T.n_tiles += int64_t(R.tile_size.size());
		T.n_slots += int64_t(R.slot_key.size()); // (the runs' are added by the caller)
		T.n_tile_points += int64_t(R.tile_lm.size());
		T.n_tile_pairs += int64_t(R.lm_slot.size());
	}
	return true;
}

// ---------------------------------------------------------------------------------------------
// the tile kernel's tables and the reduce lists
// ---------------------------------------------------------------------------------------------

// the pieces' tiles behind each other; where a tile landmark's slots start (they were appended in tile order: only the
// start of a range is ever read); the tiles' landmarks join the runs' in T.handled
void concatenate_tiles(SchurTileTables &T, const SchurStructure &s)
{
	T.tile_ptr.assign(1, 0);
	T.tile_slot_ptr.assign(1, T.n_run_slots);
	T.pair_ptr.assign(size_t(s.np + 1), 0);
	T.tile_lm.reserve(size_t(T.n_tile_points));
	T.slot_key.reserve(size_t(T.n_slots));
	T.lm_slot.reserve(size_t(T.n_tile_pairs - T.n_run_pairs));
	for(const TTileRun &R : T.tile_pieces) {
		for(size_t i = 0; i < R.tile_size.size(); ++ i) {
			T.tile_ptr.push_back(T.tile_ptr.back() + R.tile_size[i]);
			T.tile_slot_ptr.push_back(T.tile_slot_ptr.back() + R.tile_slots[i]);
		}
		T.tile_lm.insert(T.tile_lm.end(), R.tile_lm.begin(), R.tile_lm.end());
		T.slot_key.insert(T.slot_key.end(), R.slot_key.begin(), R.slot_key.end());
		T.lm_slot.insert(T.lm_slot.end(), R.lm_slot.begin(), R.lm_slot.end());
	}
	int64_t n_off = 0;
	for(size_t i = 0; i < T.tile_lm.size(); ++ i) {
		const int64_t pt = T.tile_lm[i], k = s.n_K(pt);
		T.pair_ptr[pt] = n_off;
		n_off += k * (k + 1) / 2;
		T.handled[pt] = 1;
	}
	T.pair_ptr[s.np] = n_off;
}

// key -> block of S: a table over all camera pairs where that is small (a binary search per partial block and per
// contribution of the list landmarks was a third of the analysis of the Venice-like leg), else bisection of the sorted keys
void index_blocks_of_S(SchurTileTables &T, int64_t nc, const std::vector<int32_t> &sb_row, const std::vector<int32_t> &sb_col)
{
	const int64_t n_sblocks = int64_t(sb_row.size());
	T.sb_keys.resize(size_t(n_sblocks));
	for(int64_t i = 0; i < n_sblocks; ++ i)
		T.sb_keys[i] = int64_t(sb_col[i]) * nc + sb_row[i];
	if(nc * nc <= (int64_t(1) << 24)) {
		T.key_sb.assign(size_t(nc * nc), -1);
		for(int64_t i = 0; i < n_sblocks; ++ i)
			T.key_sb[T.sb_keys[i]] = int32_t(i);
	}
}

// the partial blocks of every block of S that has some, ascending
void build_reduce_lists(SchurTileTables &T)
{
	const int64_t n_slots = T.n_slots, n_sblocks = int64_t(T.sb_keys.size());
	std::vector<int32_t> slot_sb(n_slots);
	std::vector<int64_t> sb_cnt(n_sblocks + 1, 0);
	for(int64_t g = 0; g < n_slots; ++ g) {
		const size_t k = T.n_Block_Of(T.slot_key[g]);
		if(k == T.sb_keys.size())
			throw std::logic_error("reduced camera system: a partial block is not in the block list");
		slot_sb[g] = int32_t(k);
		++ sb_cnt[k + 1];
	}
	T.rb_ptr.assign(1, 0);
	T.rb_part.resize(size_t(n_slots));
	std::vector<int64_t> start(n_sblocks, -1);
	for(int64_t b = 0; b < n_sblocks; ++ b) {
		if(sb_cnt[b + 1]) {
			start[b] = T.rb_ptr.back();
			T.rb_sb.push_back(int32_t(b));
			T.rb_ptr.push_back(T.rb_ptr.back() + sb_cnt[b + 1]);
		}
	}
	for(int64_t g = 0; g < n_slots; ++ g) // ascending partial index inside every list
		T.rb_part[start[slot_sb[g]] ++] = int32_t(g);
	T.n_rb = int64_t(T.rb_sb.size());
}

void report_reduce_lists(const SchurTileTables &T, const std::vector<int32_t> &sb_row, const std::vector<int32_t> &sb_col)
{
	int64_t n_longest_list = 0;
	std::map<int64_t, int64_t> lengths[2]; // partial blocks of a block of S -> blocks, off the diagonal and on it
	for(size_t b = 0; b + 1 < T.rb_ptr.size(); ++ b) {
		n_longest_list = std::max(n_longest_list, T.rb_ptr[b + 1] - T.rb_ptr[b]);
		++ lengths[sb_row[T.rb_sb[b]] == sb_col[T.rb_sb[b]]][T.rb_ptr[b + 1] - T.rb_ptr[b]];
	}
	fprintf(stderr, "[schur report] reduce: blocks=%lld longest=%lld off_diagonal=", (long long)T.n_rb, (long long)n_longest_list);
	report_counts(lengths[0], " diagonal=");
	report_counts(lengths[1]);
}

} // namespace

// ---------------------------------------------------------------------------------------------
// the three steps
// ---------------------------------------------------------------------------------------------

bool schur_tile_routes(SchurTileTables &T, int n_mode, const SchurStructure &s)
{
	const int64_t np = s.np;
	if(n_mode == 0 || !np || np > INT32_MAX)
		return false;
	const bool b_use_runs = n_mode != 2, b_use_tiles = n_mode != 3;
	const int64_t n_min_run = (n_mode == 3)? 1 : (n_mode == 1)? 2 : 4;
	for(int64_t pt = 0; pt < np; ++ pt) {
		const int64_t k = s.n_K(pt);
		T.n_all_pairs += k * (k + 1) / 2;
	}
	T.b_timing = getenv("SLAMPP_HIP_PLAN_TIMING") != 0;
	T.t_phase = wall_ms();
	T.handled.assign(size_t(np), 0);
	T.p_runs = std::make_shared<SchurRunTables>();
	const bool b_no_run_possible = b_use_runs && find_runs(T, s, n_min_run);
	T.Phase("runs -> jobs");
	T.n_run_slots = int64_t(T.slot_key.size());
	T.n_run_points = int64_t(T.p_runs->run_lm.size());
	if(b_use_tiles && T.n_run_points < np && !find_tiles(T, n_mode, s)) {
		T.Phase("tiles (sample)");
		return keep_lists(T, "sample");
	}
	T.Phase("tiles");
	T.n_slots += T.n_run_slots;
	const bool b_no_jobs = !T.n_tiles && T.p_runs->jobs.empty();
	if(b_no_jobs)
		return keep_lists(T, b_no_run_possible? "runs_impossible" : "no_jobs");
	if(T.n_slots > INT32_MAX)
		return keep_lists(T, "partial_block_count");
	if(n_mode < 0 && 2 * (T.n_tile_pairs + T.n_run_pairs) < T.n_all_pairs)
		return keep_lists(T, "under_half");
	T.n_list_points = np - T.n_tile_points - T.n_run_points;
	T.n_tile_pairs += T.n_run_pairs;
	return true;
}

void schur_tile_reduce_lists(SchurTileTables &T, const SchurStructure &s, const std::vector<int32_t> &sb_row, const std::vector<int32_t> &sb_col)
{
	for(const TTileRun &R : T.tile_pieces) {
		for(size_t i = 0; i < R.tile_slots.size(); ++ i)
			T.n_max_slots = std::max<int64_t>(T.n_max_slots, R.tile_slots[i]);
		for(size_t i = 0; i < R.tile_lm.size(); ++ i)
			T.n_max_k = std::max<int64_t>(T.n_max_k, s.n_K(R.tile_lm[i]));
	}
	if(T.b_timing)
		schur_tile_report(T, s);
	concatenate_tiles(T, s);
	index_blocks_of_S(T, s.nc, sb_row, sb_col);
	build_reduce_lists(T);
	if(T.b_timing)
		report_reduce_lists(T, sb_row, sb_col);
	T.Phase("partial block lists");
}

void schur_tile_report(const SchurTileTables &T, const SchurStructure &s)
{
	fprintf(stderr, "[schur] of %lld landmarks %lld in runs (%zu jobs), %lld in %lld tiles (largest %lld blocks); %lld partial blocks; "
		"%lld of %lld contributions\n", (long long)s.np, (long long)T.n_run_points, T.p_runs->jobs.size(), (long long)T.n_tile_points,
		(long long)T.n_tiles, (long long)T.n_max_slots, (long long)T.n_slots, (long long)T.n_tile_pairs, (long long)T.n_all_pairs);
	// one line per run launch that has jobs, in the order of tiles_enqueue_t; the quad flag is the enqueue's own rule
	for(int d = 1; d >= 0; -- d) {
		for(int nt = 1; nt <= 4; ++ nt) {
			for(int x = 0; x < 2; ++ x) {
				if(!T.n_run_jobs[nt][d][x])
					continue;
				int32_t n_max_points = 0;
				const TRunJob *p_job = T.p_runs->jobs.data() + T.n_run_job_first[nt][d][x];
				std::map<int32_t, int64_t> points; // landmarks of a job -> jobs
				for(int64_t j = 0; j < T.n_run_jobs[nt][d][x]; ++ j) {
					n_max_points = std::max(n_max_points, p_job[j].n_points);
					++ points[p_job[j].n_points];
				}
				fprintf(stderr, "[schur report] runs: NT=%d diag=%d prefix=%d quad=%d jobs=%lld max_points=%d points=", nt, d, x,
					int(run_launch_quad(nt, d != 0)), (long long)T.n_run_jobs[nt][d][x], int(n_max_points));
				report_counts(points);
			}
		}
	}
	if(T.n_tiles) {
		int32_t n_max_tile_points = 0;
		for(const TTileRun &R : T.tile_pieces) {
			for(size_t i = 0; i < R.tile_size.size(); ++ i)
				n_max_tile_points = std::max(n_max_tile_points, R.tile_size[i]);
		}
		fprintf(stderr, "[schur report] tiles: NL=%d tiles=%lld max_slots=%lld max_k=%lld max_points=%d\n", tile_launch_loads(s.DC, s.DP, T.n_max_k),
			(long long)T.n_tiles, (long long)T.n_max_slots, (long long)T.n_max_k, int(n_max_tile_points));
	}
	fprintf(stderr, "[schur report] routes: runs=%lld prefix=%lld tiles=%lld lists=%lld\n", (long long)T.n_run_points,
		(long long)T.n_prefix_points, (long long)T.n_tile_points, (long long)T.n_list_points);
}

void schur_run_records(int64_t *p_rec, const int32_t *p_lm, int64_t n, const SchurStructure &s)
{
	const int64_t ubase = s.n_ablocks * s.DC * s.DC, BLK = s.DC * s.DP, PP = s.DP * s.DP;
	// (a read of ptr[] per landmark, in hash order: a few threads)
	for_ranges(0, n, host_thread_count(n, 65536), [=](int, int64_t n_first, int64_t n_last) {
		for(int64_t i = n_first; i < n_last; ++ i) {
			const int64_t pt = p_lm[i];
			p_rec[i] = ubase + s.n_First_Obs(pt) * BLK + pt * PP;
		}
	});
}

// The landmarks that stay with the contribution lists: lists of their own, for the blocks of S they touch, and their
// observations by camera.  Two passes over them (count, fill), each cut into landmark ranges for a few threads: thread t's
// entries of a list follow those of thread t - 1, so every list comes out in (landmark, a, b) order, as a serial pass
// would leave it (the Venice-like leg: 3.6 M entries, 40 ms as one pass through an intermediate array, a quarter of
// the whole analysis)
void schur_tile_xlists(SchurTileTables &T, const SchurStructure &s)
{
	if(T.n_list_points <= 0)
		return;
	const int64_t nc = s.nc, n_sblocks = int64_t(T.sb_keys.size());
	const int64_t ubase = s.n_ablocks * s.DC * s.DC, BLK = s.DC * s.DP, PP = s.DP * s.DP;
	std::vector<int32_t> &list_points = T.xpoints;
	for(int64_t pt = 0; pt < s.np; ++ pt) {
		if(!T.handled[pt])
			list_points.push_back(int32_t(pt));
	}
	const int64_t n_list = int64_t(list_points.size());
	const int n_workers = host_thread_count(n_list, 2048);
	std::vector<std::vector<int64_t> > cnt_t(n_workers, std::vector<int64_t>(size_t(n_sblocks), 0)), cam_t(n_workers, std::vector<int64_t>(size_t(nc), 0));
	std::atomic<int> n_missing(0);
	for_ranges(0, n_list, n_workers, [&](int t, int64_t n_first, int64_t n_last) {
		for(int64_t i = n_first; i < n_last; ++ i) {
			const int64_t pt = list_points[i], k = s.n_K(pt);
			const int32_t *p_cam = s.p_Cams(pt);
			for(int64_t a = 0; a < k; ++ a) {
				++ cam_t[t][p_cam[a]];
				for(int64_t b = a; b < k; ++ b) {
					const size_t sb = T.n_Block_Of(int64_t(p_cam[a]) * nc + p_cam[b]);
					if(sb == T.sb_keys.size())
						++ n_missing;
					else
						++ cnt_t[t][sb];
				}
			}
		}
	});
	if(n_missing.load())
		throw std::logic_error("reduced camera system: a contribution's block is not in the block list");
	T.xsb_ptr.push_back(0);
	std::vector<int64_t> start(n_sblocks, -1);
	for(int64_t b = 0; b < n_sblocks; ++ b) {
		int64_t n_total = 0;
		for(int t = 0; t < n_workers; ++ t)
			n_total += cnt_t[t][b];
		if(n_total) {
			start[b] = T.xsb_ptr.back();
			T.xsb_map.push_back(int32_t(b));
			T.xsb_ptr.push_back(T.xsb_ptr.back() + n_total);
		}
		int64_t n_at = start[b];
		for(int t = 0; t < n_workers; ++ t) { // cnt_t[t][b] becomes where thread t's entries of list b start
			const int64_t n_mine = cnt_t[t][b];
			cnt_t[t][b] = n_at;
			n_at += n_mine;
		}
	}
	T.xcam_ptr.assign(nc + 1, 0);
	for(int64_t c = 0; c < nc; ++ c) {
		int64_t n_at = T.xcam_ptr[c];
		for(int t = 0; t < n_workers; ++ t) {
			const int64_t n_mine = cam_t[t][c];
			cam_t[t][c] = n_at;
			n_at += n_mine;
		}
		T.xcam_ptr[c + 1] = n_at;
	}
	T.xent_a.resize(size_t(T.xsb_ptr.back()));
	T.xent_uoff.resize(size_t(T.xsb_ptr.back()));
	T.xcam_obs.resize(size_t(T.xcam_ptr[nc]));
	for_ranges(0, n_list, n_workers, [&](int t, int64_t n_first, int64_t n_last) {
		for(int64_t i = n_first; i < n_last; ++ i) {
			const int64_t pt = list_points[i], k = s.n_K(pt), o0 = s.n_First_Obs(pt);
			const int32_t *p_cam = s.p_Cams(pt);
			for(int64_t a = 0; a < k; ++ a) {
				T.xcam_obs[size_t(cam_t[t][p_cam[a]] ++)] = int32_t(o0 + a);
				for(int64_t b = a; b < k; ++ b) {
					const size_t sb = T.n_Block_Of(int64_t(p_cam[a]) * nc + p_cam[b]);
					const int64_t d = cnt_t[t][sb] ++;
					T.xent_a[size_t(d)] = int32_t(o0 + a);
					// the U block of observation b: the values hold [U .. U | C] per landmark
					T.xent_uoff[size_t(d)] = ubase + (o0 + b) * BLK + pt * PP;
				}
			}
		}
	});
}

// ---------------------------------------------------------------------------------------------
// contributions to S grouped by block
// ---------------------------------------------------------------------------------------------

// Which blocks of S exist: a bit per camera pair, a bitmap per thread over its range of landmarks, OR-ed at the end
// (counting the contributions of every block was 19 ms on one core at C5 -- with atomic adds from eight, every landmark of
// the band structure on the same few thousand counters, 88 ms --, and the counts are only needed where the landmarks cannot
// be taken one by one: schur_lists_by_counting)
void schur_blocks_from_bitmap(std::vector<int32_t> &sb_row, std::vector<int32_t> &sb_col, const SchurStructure &s,
	const raw_vector<int32_t> &obs_cam, int n_workers)
{
	const int64_t nc = s.nc, n_words = (nc * nc + 63) / 64;
	std::vector<std::vector<uint64_t> > pair_bits(n_workers, std::vector<uint64_t>(size_t(n_words), 0));
	for_ranges(0, s.np, n_workers, [&](int t, int64_t n_first, int64_t n_last) {
		std::vector<uint64_t> &r_bits = pair_bits[t];
		for(int64_t pt = n_first; pt < n_last; ++ pt) {
			const int64_t o0 = s.n_First_Obs(pt), o1 = s.n_First_Obs(pt + 1);
			for(int64_t a = o0; a < o1; ++ a) {
				const int64_t n_base = int64_t(obs_cam[a]) * nc;
				for(int64_t b = a; b < o1; ++ b) {
					const int64_t key = n_base + obs_cam[b];
					r_bits[size_t(key >> 6)] |= uint64_t(1) << (key & 63);
				}
			}
		}
	});
	for(int64_t w = 0; w < n_words; ++ w) {
		uint64_t n_word = 0;
		for(int t = 0; t < n_workers; ++ t)
			n_word |= pair_bits[t][size_t(w)];
		for(; n_word; n_word &= n_word - 1) {
			const int64_t key = w * 64 + __builtin_ctzll(n_word);
			sb_col.push_back(int32_t(key / nc));
			sb_row.push_back(int32_t(key % nc));
		}
	}
}

// A counter array per thread over its range of landmarks (one thread counted and placed the five million contributions of
// the uniform-visibility C4 in 37 ms); every contribution lands where a serial pass would put it: inside a block in
// landmark order
void schur_lists_by_counting(std::vector<int64_t> &sb_ptr, raw_vector<int32_t> &ent_a, raw_vector<int64_t> &ent_uoff,
	const SchurStructure &s, const raw_vector<int32_t> &obs_cam, int64_t n_entries, size_t n_sblocks, int n_workers)
{
	const int64_t nc = s.nc, np = s.np, n_keys = nc * nc;
	const int64_t ubase = s.n_ablocks * s.DC * s.DC, BLK = s.DC * s.DP, PP = s.DP * s.DP;
	const int n_list_workers = int(std::max<int64_t>(1, std::min<int64_t>(n_workers, (int64_t(1) << 26) / std::max<int64_t>(n_keys, 1)))); // (at most 512 MB of counters)
	std::vector<raw_vector<int64_t> > cnt(n_list_workers);
	for_ranges(0, np, n_list_workers, [&](int t, int64_t n_first, int64_t n_last) {
		raw_vector<int64_t> &r_cnt = cnt[t];
		r_cnt.assign(size_t(n_keys), 0);
		for(int64_t pt = n_first; pt < n_last; ++ pt) {
			const int64_t o0 = s.n_First_Obs(pt), o1 = s.n_First_Obs(pt + 1);
			for(int64_t a = o0; a < o1; ++ a)
				for(int64_t b = a; b < o1; ++ b)
					++ r_cnt[int64_t(obs_cam[a]) * nc + obs_cam[b]];
		}
	});
	// where every thread's contributions to every block start: block by block, inside a block thread by thread --
	// the ranges of blocks first by themselves, then shifted by what the ranges before them hold
	std::vector<int64_t> range_total(n_list_workers, 0);
	std::vector<std::vector<int64_t> > range_starts(n_list_workers); // start of every nonzero block of the range
	for_ranges(0, n_keys, n_list_workers, [&](int r, int64_t n_first, int64_t n_last) {
		int64_t n_sum = 0;
		for(int64_t key = n_first; key < n_last; ++ key) {
			const int64_t n_before = n_sum;
			for(int t = 0; t < n_list_workers; ++ t) {
				const int64_t n_here = cnt[t][size_t(key)];
				cnt[t][size_t(key)] = n_sum;
				n_sum += n_here;
			}
			if(n_sum != n_before)
				range_starts[r].push_back(n_before);
		}
		range_total[r] = n_sum;
	});
	std::vector<int64_t> range_base(n_list_workers + 1, 0);
	for(int r = 0; r < n_list_workers; ++ r)
		range_base[r + 1] = range_base[r] + range_total[r];
	for_ranges(0, n_keys, n_list_workers, [&](int r, int64_t n_first, int64_t n_last) {
		if(!range_base[r])
			return;
		for(int t = 0; t < n_list_workers; ++ t) {
			int64_t *p_cnt = cnt[t].data();
			for(int64_t key = n_first; key < n_last; ++ key)
				p_cnt[key] += range_base[r];
		}
	});
	for(int r = 0; r < n_list_workers; ++ r) {
		for(size_t i = 0; i < range_starts[r].size(); ++ i)
			sb_ptr.push_back(range_starts[r][i] + range_base[r]);
	}
	sb_ptr.push_back(n_entries);
	if(sb_ptr.size() != n_sblocks + 1 || range_base[n_list_workers] != n_entries)
		throw std::logic_error("reduced camera system: the block list and the contribution counts disagree");
	ent_a.resize(n_entries);
	ent_uoff.resize(n_entries);
	for_ranges(0, np, n_list_workers, [&](int t, int64_t n_first, int64_t n_last) {
		int64_t *p_fill = cnt[t].data();
		for(int64_t pt = n_first; pt < n_last; ++ pt) {
			const int64_t o0 = s.n_First_Obs(pt), o1 = s.n_First_Obs(pt + 1);
			for(int64_t a = o0; a < o1; ++ a)
				for(int64_t b = a; b < o1; ++ b) {
					const int64_t d = p_fill[int64_t(obs_cam[a]) * nc + obs_cam[b]] ++;
					ent_a[d] = int32_t(a);
					ent_uoff[d] = ubase + b * BLK + pt * PP;
				}
		}
	});
}

void schur_lists_by_sorting(std::vector<int64_t> &sb_ptr, std::vector<int32_t> &sb_row, std::vector<int32_t> &sb_col,
	raw_vector<int32_t> &ent_a, raw_vector<int64_t> &ent_uoff, const SchurStructure &s, const raw_vector<int32_t> &obs_cam,
	const raw_vector<int32_t> &obs_pt, int64_t n_entries)
{
	const int64_t nc = s.nc;
	const int64_t ubase = s.n_ablocks * s.DC * s.DC, BLK = s.DC * s.DP, PP = s.DP * s.DP;
	ent_a.resize(n_entries);
	ent_uoff.resize(n_entries);
	struct TE { int64_t key; int32_t a, b; };
	std::vector<TE> ents(n_entries);
	int64_t e = 0;
	for(int64_t pt = 0; pt < s.np; ++ pt) {
		const int64_t o0 = s.n_First_Obs(pt), o1 = s.n_First_Obs(pt + 1);
		for(int64_t a = o0; a < o1; ++ a)
			for(int64_t b = a; b < o1; ++ b) {
				ents[e].key = int64_t(obs_cam[a]) * nc + obs_cam[b];
				ents[e].a = int32_t(a);
				ents[e].b = int32_t(b);
				++ e;
			}
	}
	std::sort(ents.begin(), ents.end(), [](const TE &x, const TE &y) {
		return x.key < y.key || (x.key == y.key && x.a < y.a); });
	for(e = 0; e < n_entries; ++ e) {
		if(!e || ents[e].key != ents[e - 1].key) {
			sb_ptr.push_back(e);
			sb_col.push_back(int32_t(ents[e].key / nc));
			sb_row.push_back(int32_t(ents[e].key % nc));
		}
		ent_a[e] = ents[e].a;
		ent_uoff[e] = ubase + int64_t(ents[e].b) * BLK + int64_t(obs_pt[ents[e].b]) * PP;
	}
	sb_ptr.push_back(n_entries);
}

} // namespace slampp
