// tile_schedule.cpp -- the tables of the dense top's tile schedule (tile_schedule.h); the kernels that run them are in
// dense_tiles.hip
#include "tile_schedule.h"
#include "plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace slampp {

bool tile_schedule_tables(int n_tile_num, const std::vector<char> &r_nonzero, int n_rider_chunk, int n_rider_budget,
	TTileTables &r_t)
{
	typedef TTileRec4 int4;
	typedef TTileRec2 int2;
	r_t = TTileTables();
	const int T = n_tile_num;
	if(T <= 0 || r_nonzero.size() != size_t(T) * T)
		return false;
	// structure of the tile factor: symbolic elimination at tile granularity (the block-level structure it comes
	// from is already closed; whole tiles are not, e.g. two blocks of different columns sharing a tile column)
	std::vector<char> nz(r_nonzero);
	for(int j = 0; j < T; ++ j) {
		nz[size_t(j) + size_t(j) * T] = 1;
		nz[size_t(T - 1) + size_t(j) * T] = 1; // the right-hand side rides in the last row
	}
	r_t.height = tile_symbolic(T, nz);
	const std::vector<int> &height = r_t.height;
	const int n_max_height = *std::max_element(height.begin(), height.end());
	const int n_levels = n_max_height + 1;
	r_t.n_tiles = T;
	r_t.n_levels = n_levels;
	std::vector<int> &potrf = r_t.potrf;
	std::vector<int4> &trsm = r_t.trsm; // (row tile, column tile, also updates the diagonal tile of its row, -)
	std::vector<int4> &tgt = r_t.tgt;   // per level: first the urgent targets (diagonal tiles of the next level's columns), then the others
	std::vector<int> &src = r_t.src;
	std::vector<int> &level_potrf_ptr = r_t.level_potrf_ptr, &level_trsm_ptr = r_t.level_trsm_ptr,
		&level_tgt_ptr = r_t.level_tgt_ptr, &level_urgent_end = r_t.level_urgent_end, &rider_ptr = r_t.rider_ptr;
	level_potrf_ptr.assign(1, 0);
	level_trsm_ptr.assign(1, 0);
	level_tgt_ptr.assign(1, 0);
	level_urgent_end.clear();
	std::vector<int> tgt_of(size_t(T) * T, -1); // per level: index (in `found`) of the target record of a tile
	// updates nothing in the next level waits for ("riders": extra workgroups of the diagonal-tile launches): per target tile
	// its deadline -- the last diagonal launch it may ride in -- and its sources (level they become available after, column)
	struct TPending { int i1, i2, n_deadline; size_t n_done; std::vector<int2> sources; };
	std::vector<TPending> pending;
	std::vector<int> pending_of(size_t(T) * T, -1);
	for(int l = 0; l < n_levels; ++ l) {
		std::vector<int2> found;                 // targets of this level
		std::vector<std::vector<int> > sources;  // per target
		const size_t n_trsm0 = trsm.size();
		for(int j = 0; j < T; ++ j) {
			if(height[j] != l)
				continue;
			potrf.push_back(j);
			for(int i = j + 1; i < T; ++ i) {
				if(nz[size_t(i) + size_t(j) * T])
					trsm.push_back(int4{i, j, 0, 0});
			}
			for(int i2 = j + 1; i2 < T; ++ i2) {
				if(!nz[size_t(i2) + size_t(j) * T])
					continue;
				for(int i1 = i2; i1 < T; ++ i1) {
					if(!nz[size_t(i1) + size_t(j) * T])
						continue;
					int &r_idx = tgt_of[size_t(i1) + size_t(i2) * T];
					if(r_idx < 0) {
						r_idx = int(found.size());
						found.push_back(int2{i1, i2});
						sources.push_back(std::vector<int>());
					}
					sources[r_idx].push_back(j);
				}
			}
		}
		// what the next level's diagonal tiles wait for: with a single source, the panel solve of that source does it
		// on its way; with several, an update launch of its own; everything else rides in the next level's first launch
		std::vector<int> urgent, deferred;
		for(size_t k = 0; k < found.size(); ++ k) {
			const int i1 = found[k].x, i2 = found[k].y;
			tgt_of[size_t(i1) + size_t(i2) * T] = -1; // (for the next level)
			const bool b_next_diag = i1 == i2 && height[i1] == l + 1;
			if(b_next_diag && sources[k].size() == 1) {
				bool b_found = false;
				for(size_t p = n_trsm0; p < trsm.size() && !b_found; ++ p) {
					if(trsm[p].x == i1 && trsm[p].y == sources[k][0]) {
						trsm[p].z = 1;
						b_found = true;
					}
				}
				if(!b_found)
					return false; // (cannot happen: the source tile is a panel tile of this level)
			} else
				(b_next_diag? urgent : deferred).push_back(int(k));
		}
		for(size_t q = 0; q < urgent.size(); ++ q) {
			const int k = urgent[q];
			int4 t = {found[k].x, found[k].y, int(src.size()), 0};
			src.insert(src.end(), sources[k].begin(), sources[k].end());
			t.w = int(src.size());
			tgt.push_back(t);
		}
		level_urgent_end.push_back(int(tgt.size()));
		for(size_t q = 0; q < deferred.size(); ++ q) { // not wanted by the next level: to the pool of riders, scheduled below
			const int k = deferred[q], i1 = found[k].x, i2 = found[k].y;
			int &r_id = pending_of[size_t(i1) + size_t(i2) * T];
			if(r_id < 0) {
				r_id = int(pending.size());
				// a sub-diagonal tile is read by the panel solves of its column's level (launched after that level's diagonal
				// tiles: it may still ride with those), a diagonal tile by the diagonal launch of its level
				pending.push_back(TPending{i1, i2, (i1 == i2)? height[i2] - 1 : height[i2], 0, std::vector<int2>()});
			}
			for(size_t e = 0; e < sources[k].size(); ++ e)
				pending[r_id].sources.push_back(int2{l, sources[k][e]});
		}
		level_potrf_ptr.push_back(int(potrf.size()));
		level_trsm_ptr.push_back(int(trsm.size()));
		level_tgt_ptr.push_back(int(tgt.size()));
	}
	// The riders, launch by launch.  Until round 5 every update rode in the very next diagonal launch: at the Venice-like C4's
	// reduced system the first launches carried 300 - 600 jobs of several source tiles each and lasted 25 - 50 us where the
	// diagonal tile needs 13 (150 us of a 0.79 ms solve), while from the tenth level on the chip idled beside one tile.  Now an
	// update may ride in any diagonal launch between the level that produced its sources and its deadline: every launch
	// takes what is due, then the most urgent of the rest up to a budget of source tiles, at most TILE_RIDER_CHUNK sources
	// of a target at a time (a job lasts as long as its list) -- one job per target and launch, sources in level order: the
	// sums keep a fixed order.
	const int TILE_RIDER_CHUNK = n_rider_chunk, TILE_RIDER_BUDGET = n_rider_budget;
	std::vector<int4> &riders = r_t.riders;
	rider_ptr.assign(2, 0); // (no riders in the first level's launch)
	{
		std::vector<int> order(pending.size());
		for(size_t i = 0; i < order.size(); ++ i)
			order[i] = int(i);
		std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pending[a].n_deadline < pending[b].n_deadline; });
		for(int lv = 1; lv < n_levels; ++ lv) {
			int n_budget = TILE_RIDER_BUDGET;
			for(int n_pass = 0; n_pass < 2; ++ n_pass) { // what is due first, then by deadline
				for(size_t q = 0; q < order.size(); ++ q) {
					TPending &r_p = pending[order[q]];
					const bool b_due = r_p.n_deadline <= lv;
					if(b_due != !n_pass || r_p.n_done == r_p.sources.size() || r_p.n_done == size_t(-1))
						continue;
					size_t n_avail = 0; // sources of levels below this launch's, not applied yet
					while(r_p.n_done + n_avail < r_p.sources.size() && r_p.sources[r_p.n_done + n_avail].x < lv)
						++ n_avail;
					if(!n_avail)
						continue;
					if(!b_due) {
						if(n_budget <= 0)
							continue;
						n_avail = std::min<size_t>(n_avail, size_t(TILE_RIDER_CHUNK));
					}
					int4 t = {r_p.i1, r_p.i2, int(src.size()), 0};
					for(size_t e = 0; e < n_avail; ++ e)
						src.push_back(r_p.sources[r_p.n_done + e].y);
					t.w = int(src.size());
					riders.push_back(t);
					r_p.n_done += n_avail;
					n_budget -= int(n_avail);
				}
			}
			if(getenv("SLAMPP_HIP_PLAN_TIMING")) { // development aid: what rides where
				int n_src_here = 0;
				for(size_t i = size_t(rider_ptr.back()); i < riders.size(); ++ i)
					n_src_here += riders[i].w - riders[i].z;
				fprintf(stderr, "[tiles] level %2d: %3d diagonal tiles, %4d riders with %5d source tiles\n", lv,
					level_potrf_ptr[lv + 1] - level_potrf_ptr[lv], int(riders.size()) - rider_ptr.back(), n_src_here);
			}
			rider_ptr.push_back(int(riders.size()));
		}
		if(n_levels < 2)
			rider_ptr.assign(size_t(n_levels) + 1, 0);
		for(size_t i = 0; i < pending.size(); ++ i) {
			if(pending[i].n_done != pending[i].sources.size())
				return false; // (cannot happen: a source's level is below its target's deadline)
		}
	}
	// the backward substitution, top down.  The ancestors of a tile column (the rows of its nonzero tiles) all have
	// different heights (two of them are linked by fill), so a column gets at most one contribution per launch: from the
	// ancestor of height h + 1 by the launch of height h -- in the column's own workgroup if h is its own height, by a
	// carrying workgroup otherwise.  z_k starts as y_k, which lives in the last row of the factor: the first workgroup to
	// touch z_k takes it from there
	std::vector<int4> &back_diag = r_t.back_diag, &back_carry = r_t.back_carry;
	std::vector<int> &back_diag_ptr = r_t.back_diag_ptr, &back_carry_ptr = r_t.back_carry_ptr;
	back_diag_ptr.assign(1, 0);
	back_carry_ptr.assign(1, 0);
	{
		std::vector<char> touched(T, 0);
		for(int h = n_max_height; h >= 0; -- h) {
			for(int k = 0; k < T; ++ k) {
				if(height[k] > h)
					continue;
				int n_up = -1; // the ancestor of height h + 1
				for(int j = k + 1; j < T && n_up < 0; ++ j) {
					if(nz[size_t(j) + size_t(k) * T] && height[j] == h + 1)
						n_up = j;
				}
				if(height[k] == h)
					back_diag.push_back(int4{k, n_up, !touched[k], 0});
				else if(n_up >= 0) {
					back_carry.push_back(int4{n_up, k, !touched[k], 0});
					touched[k] = 1;
				}
			}
			back_diag_ptr.push_back(int(back_diag.size()));
			back_carry_ptr.push_back(int(back_carry.size()));
		}
	}
	return true;
}

} // namespace slampp
