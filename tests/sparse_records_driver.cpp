// Test infrastructure (tests/test_sparse_records_sanitizers.py): the host record builders of the sparse block path
// (csrc/sparse_records.cpp) on small graphs, in the order the analysis runs them, every array they lay out decoded again
// and checked against the plan.  Built with AddressSanitizer + UBSan on the CPU; nothing here touches a device.
// Prints one line per case ("<name>: reached <branches> ok") and exits 0, or says what is wrong and exits 1.
#include "sparse_records.h"
#include "driver_graphs.h"
#include <cstring>
#include <map>
#include <string>
using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: failed: %s (line %d)\n", name, #cond, __LINE__); return false; } } while(0)

struct TCase {
	SparseRecordOptions opt;
	Plan P;
	SparseRecords R;
	SparseLaunchLists L;
	std::set<std::string> reached;
};

// a decoded panel package
struct TPackage {
	TPanelHead hd;
	std::vector<TPanelCol> cols;
	std::vector<TPanelSlot> slots;
	std::vector<uint32_t> irow, ipair;
	std::vector<TPanelExt> fresh;
	std::vector<int64_t> blk; // slot -> factor block
	int n_stage, n_task;
	// its hand-up list
	std::vector<TPanelOut> out;
	std::vector<uint32_t> out_pairs;
};

template <class T>
static bool read_units(const raw_vector<longlong2> &v, size_t n_unit, size_t n, std::vector<T> &r_out)
{
	const size_t n_bytes = n * sizeof(T);
	if(n_unit * 16 + n_bytes > v.size() * 16)
		return false;
	r_out.resize(n);
	if(n)
		memcpy(r_out.data(), reinterpret_cast<const char*>(v.data()) + n_unit * 16, n_bytes);
	return true;
}

// the builders in the analysis' order: upper column records, panel packages (the rest of the records not written yet, as
// when they are built beside them), remaining records, column packages, dense top, lane-per-task tables
static void build_all(TCase &c)
{
	const Plan &P = c.P;
	c.L.n_bottom_stages = count_bottom_stages(P, c.opt);
	alloc_column_records(P, c.R);
	const int64_t n_upper_begin = first_upper_column(P, c.opt, c.L), n_sched = int64_t(c.R.cols.size());
	if(!c.R.cols.empty())
		memset(c.R.cols.data(), 0xee, c.R.cols.size() * sizeof(TColDesc)); // (what the package builder must not read)
	if(!c.R.blks.empty())
		memset(c.R.blks.data(), 0xee, c.R.blks.size() * sizeof(TBlkDesc));
	if(!c.R.rents.empty())
		memset(c.R.rents.data(), 0xee, c.R.rents.size() * sizeof(TRowEnt));
	fill_column_records(P, c.R, n_upper_begin, n_sched);
	reserve_panel_packages(P, c.L, n_upper_begin, c.R);
	build_panel_packages(P, c.opt, c.R, c.L);
	Parallel_Ranges(n_upper_begin, 64, [&](int64_t b, int64_t e) { fill_column_records(P, c.R, b, e); }, 4);
	fill_dense_top_column_records(P, c.R);
	build_column_packages(P, c.L, c.R);
	build_dense_top_records(P, P.dense_dim? (P.dense_dim + 1 + 63) / 64 * 64 : 0, c.R);
	build_simt_tables(P, c.opt, c.R, c.L);
	if(n_upper_begin > 0)
		c.reached.insert("upper_first");
}

static bool check_column_records(const char *name, TCase &c)
{
	const Plan &P = c.P;
	const SparseRecords &R = c.R;
	const int64_t n_factor = P.loff.back(), n_scalars = P.cs_new[P.n], n_lblocks = int64_t(P.lrow.size());
	const int64_t n_asrc_max = P.asrc.empty()? -1 : *std::max_element(P.asrc.begin(), P.asrc.end());
	REQUIRE(R.cols.size() == P.task_cols.size() && int64_t(R.blks.size()) == n_lblocks && R.pairs.size() == P.pa.size() && R.rents.size() == P.rblk.size());
	for(size_t i = 0; i < R.cols.size(); ++ i) {
		const TColDesc &d = R.cols[i];
		const int32_t j = P.task_cols[i];
		REQUIRE(d.k0 == P.lptr[j] && d.nb >= 1 && d.k0 + d.nb == P.lptr[j + 1] && d.dj == P.dim[j]);
		REQUIRE(d.linv_off >= 0 && d.linv_off + int64_t(d.dj) * d.dj <= P.linv_off[P.n]);
		REQUIRE(d.cs_new >= 0 && d.cs_new + d.dj <= n_scalars && d.cs_src >= 0 && d.cs_src + d.dj <= n_scalars);
		REQUIRE(d.r0 >= 0 && d.nr >= 0 && d.r0 + d.nr <= int64_t(P.rblk.size()) && d.r0 == P.rptr[j] && d.nr == P.rptr[j + 1] - P.rptr[j]);
		REQUIRE(d.p0 >= 0 && d.np >= 0 && d.p0 + d.np <= int64_t(P.pa.size()) && d.p0 + d.np == P.pptr[P.lptr[j + 1]]);
	}
	for(int64_t k = 0; k < n_lblocks; ++ k) {
		const TBlkDesc &b = R.blks[size_t(k)];
		const int di = int(b.np_di >> 24), np = int(b.np_di & 0xffffff);
		REQUIRE(b.loff == P.loff[k] && b.loff >= 0 && b.loff + int64_t(di) * P.dim[P.blk_col[k]] <= n_factor);
		REQUIRE(b.asrc >= -1 && (b.asrc >> 1) <= n_asrc_max && di == P.dim[P.lrow[k]]);
		REQUIRE(b.p0 == P.pptr[k] && b.p0 + np == P.pptr[k + 1] && b.xcs >= 0 && b.xcs + di <= n_scalars);
	}
	for(size_t e = 0; e < R.pairs.size(); ++ e) {
		const int64_t a = R.pairs[e].x & ((int64_t(1) << 48) - 1), b = R.pairs[e].y;
		REQUIRE(a == P.loff[P.pa[e]] && b == P.loff[P.pb[e]] && a < n_factor && b < n_factor);
		REQUIRE(((R.pairs[e].x >> 56) & 0xff) == P.dim[P.blk_col[P.pa[e]]]);
	}
	for(size_t e = 0; e < R.rents.size(); ++ e) {
		REQUIRE(R.rents[e].off == P.loff[P.rblk[e]] && R.rents[e].off < n_factor);
		REQUIRE(R.rents[e].ycs >= 0 && R.rents[e].ycs + R.rents[e].dc <= n_scalars && R.rents[e].dc == P.dim[P.blk_col[P.rblk[e]]]);
	}
	return true;
}

static bool check_column_packages(const char *name, TCase &c)
{
	const Plan &P = c.P;
	const SparseRecords &R = c.R;
	const int64_t n_factor = P.loff.back(), n_scalars = P.cs_new[P.n];
	const int n_stages = int(P.stage_ptr.size()) - 1;
	REQUIRE(R.task_pkg.size() == P.task_ptr.size() - 1);
	if(R.pkg.empty()) {
		for(size_t t = 0; t < R.task_pkg.size(); ++ t)
			REQUIRE(R.task_pkg[t] == -1);
		c.reached.insert("no_column_packages");
		return true;
	}
	REQUIRE(R.pkg.size() >= size_t(PKG_SPECULATIVE));
	const int64_t n_end = int64_t(R.pkg.size()) - PKG_SPECULATIVE;
	int64_t n_at = 0;
	for(int t = 0; t < int(R.task_pkg.size()); ++ t) {
		if(n_stages <= 1 || t < P.stage_ptr[1]) { // (the leaf stage has none)
			REQUIRE(R.task_pkg[size_t(t)] == -1);
			continue;
		}
		REQUIRE(R.task_pkg[size_t(t)] == n_at);
		const bool b_wide = t < P.stage_ptr[std::min(c.L.n_bottom_stages, n_stages)];
		for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i) {
			const TColDesc &d = R.cols[size_t(i)];
			REQUIRE(n_at + 4 <= n_end && !memcmp(&R.pkg[size_t(n_at)], &d, sizeof(d)));
			const bool b_fits = d.nb <= (b_wide? int(WIDE_CHUNK) : int(UP_CHUNK)) && d.nr <= (b_wide? int(WIDE_NR) : int(UP_NR)) &&
				d.np <= (b_wide? int(WIDE_NP) : int(UP_NP));
			if(!b_fits) {
				c.reached.insert(b_wide? "wide_column_over_limits" : "upper_column_over_limits");
				n_at += 4;
				continue;
			}
			const int ne = d.nr + d.np;
			REQUIRE(n_at + package_units(d.nb, ne) <= n_end);
			REQUIRE(!memcmp(&R.pkg[size_t(n_at) + 4], &R.blks[size_t(d.k0)], size_t(d.nb) * sizeof(TBlkDesc)));
			const longlong2 *p_ent = &R.pkg[size_t(n_at) + 4 + 2 * size_t(d.nb)];
			std::vector<int32_t> ycs(size_t(ne), 0);
			std::vector<unsigned char> tag(size_t(ne), 0);
			if(ne) {
				memcpy(ycs.data(), p_ent + ne, size_t(ne) * 4);
				memcpy(tag.data(), p_ent + ne + (ne + 3) / 4, size_t(ne));
			}
			for(int e = 0; e < ne; ++ e) {
				REQUIRE(p_ent[e].x >= 0 && p_ent[e].x < n_factor && p_ent[e].y >= 0 && p_ent[e].y < n_factor);
				if(e < d.nr)
					REQUIRE(p_ent[e].x == P.loff[P.rblk[d.r0 + e]] && p_ent[e].y == p_ent[e].x && ycs[size_t(e)] >= 0 && ycs[size_t(e)] < n_scalars && tag[size_t(e)] == 0);
				else
					REQUIRE(p_ent[e].x == P.loff[P.pa[d.p0 + e - d.nr]] && p_ent[e].y == P.loff[P.pb[d.p0 + e - d.nr]] && tag[size_t(e)] >= 1 && tag[size_t(e)] < d.nb);
			}
			n_at += package_units(d.nb, ne);
		}
	}
	REQUIRE(n_at == n_end);
	return true;
}

// decodes every panel package and hand-up list, checking the layout and every offset on the way
static bool decode_packages(const char *name, TCase &c, std::vector<TPackage> &pk)
{
	const Plan &P = c.P;
	const SparseRecords &R = c.R;
	const SparseLaunchLists &L = c.L;
	const int64_t n_factor = P.loff.back(), n_scalars = P.cs_new[P.n];
	const int n_stages = int(P.stage_ptr.size()) - 1, DD = P.max_dim * P.max_dim;
	std::map<int64_t, int32_t> col_of_cs;
	std::vector<int32_t> task_of_col(size_t(P.n), -1);
	for(int32_t j = 0; j < P.n; ++ j)
		col_of_cs[P.cs_new[j]] = j;
	for(int t = 0; t + 1 < int(P.task_ptr.size()); ++ t) {
		for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i)
			task_of_col[P.task_cols[i]] = t;
	}
	REQUIRE(R.panel_off.size() == R.panel_out_off.size() && R.panel_off.size() == R.panel_units.size());
	if(L.panel_ptr.empty()) {
		REQUIRE(R.panel_off.empty() && R.panel_rest.empty() && R.upd_slots.empty() && R.upd_ents.empty() && L.panel_rest_ptr.empty() && L.panel_upd_ptr.empty());
		c.reached.insert("no_panel_packages");
		return true;
	}
	REQUIRE(int(L.panel_ptr.size()) == n_stages + 1 && int(L.panel_rest_ptr.size()) == n_stages + 1 && int(L.panel_upd_ptr.size()) == n_stages + 1);
	REQUIRE(int(L.panel_cfg.size()) >= n_stages && int(L.panel_ride.size()) >= n_stages);
	REQUIRE(L.panel_ptr[0] == 0 && L.panel_rest_ptr[0] == 0 && L.panel_upd_ptr[0] == 0);
	for(int s = 0; s < n_stages; ++ s)
		REQUIRE(L.panel_ptr[s] <= L.panel_ptr[s + 1] && L.panel_rest_ptr[s] <= L.panel_rest_ptr[s + 1] && L.panel_upd_ptr[s] <= L.panel_upd_ptr[s + 1]);
	REQUIRE(L.panel_ptr.back() == int32_t(R.panel_off.size()) && L.panel_rest_ptr.back() == int32_t(R.panel_rest.size()) &&
		L.panel_upd_ptr.back() == int32_t(R.upd_slots.size()));
	REQUIRE(R.panel_pkg.size() >= size_t(64 * PANEL_W));
	const size_t n_pkg_end = R.panel_pkg.size() - 64 * PANEL_W; // (the speculative read of a workgroup stays inside)
	pk.resize(R.panel_off.size());
	for(int s = 0; s < n_stages; ++ s) {
		const TPanelLaunch &cfg = L.panel_cfg[size_t(s)];
		REQUIRE(cfg.n_waves == 2 || cfg.n_waves == 4 || cfg.n_waves == 8);
		if(L.panel_ptr[s + 1] > L.panel_ptr[s])
			REQUIRE(size_t(panel_lds(P.max_dim, true, cfg).TOTAL) * 8 <= size_t(PANEL_LDS_BUDGET));
		bool b_plan_order = true;
		for(int32_t p = L.panel_ptr[s]; p < L.panel_ptr[s + 1]; ++ p) {
			TPackage &k = pk[size_t(p)];
			k.n_stage = s;
			const int64_t n_off = R.panel_off[size_t(p)];
			REQUIRE(n_off >= 0 && size_t(n_off) + 4 <= n_pkg_end);
			b_plan_order = b_plan_order && (p == L.panel_ptr[s] || R.panel_off[size_t(p) - 1] < n_off);
			memcpy(&k.hd, &R.panel_pkg[size_t(n_off)], sizeof(TPanelHead));
			const TPanelHead &hd = k.hd;
			REQUIRE(hd.n_cols >= 1 && hd.n_cols <= int(PANEL_COLS) && hd.n_slots >= hd.n_cols && hd.n_slots <= panel_slot_cap(P.max_dim));
			REQUIRE(hd.n_units >= 4 && hd.n_units <= int(PANEL_UNITS) && size_t(n_off) + size_t(hd.n_units) <= n_pkg_end && hd.n_int_rows >= 0);
			REQUIRE(hd.n_cols <= cfg.n_cap_cols && hd.n_slots <= cfg.n_cap_blk && hd.n_units <= cfg.n_cap_units);
			size_t n_unit = size_t(n_off) + 4;
			REQUIRE(read_units(R.panel_pkg, n_unit, size_t(hd.n_cols), k.cols));
			n_unit += 3 * size_t(hd.n_cols);
			REQUIRE(read_units(R.panel_pkg, n_unit, size_t(hd.n_slots), k.slots));
			n_unit += 2 * size_t(hd.n_slots);
			REQUIRE(read_units(R.panel_pkg, n_unit, size_t(hd.n_int_rows), k.irow));
			n_unit += (size_t(hd.n_int_rows) + 3) / 4;
			int64_t n_int_pairs = 0;
			for(size_t q = 0; q < k.slots.size(); ++ q) {
				REQUIRE(k.slots[q].ip0 == n_int_pairs && k.slots[q].inp >= 0);
				n_int_pairs += k.slots[q].inp;
			}
			REQUIRE(read_units(R.panel_pkg, n_unit, size_t(n_int_pairs), k.ipair));
			n_unit += (size_t(n_int_pairs) + 3) / 4;
			REQUIRE(hd.ext_ptr[0] == 0);
			for(int v = 0; v < cfg.n_waves; ++ v)
				REQUIRE(hd.ext_ptr[v] <= hd.ext_ptr[v + 1]);
			for(int v = cfg.n_waves + 1; v < 10; ++ v)
				REQUIRE(hd.ext_ptr[v] == 0);
			const int n_fresh = hd.ext_ptr[cfg.n_waves];
			REQUIRE(read_units(R.panel_pkg, n_unit, size_t(n_fresh), k.fresh));
			n_unit += 2 * size_t(n_fresh);
			REQUIRE(n_unit == size_t(n_off) + size_t(hd.n_units)); // n_units is the size the layout occupies
			REQUIRE(R.panel_units[size_t(p)] >= 4); // (panel_units keeps the plan's order: compared as a multiset below)
			// columns and slots
			int n_slot = 0, n_irow = 0, n_level_cols = 0;
			for(int o = 0; o < hd.n_cols; ++ o) {
				const TPanelCol &pc = k.cols[size_t(o)];
				REQUIRE(col_of_cs.count(pc.cs_new));
				const int32_t j = col_of_cs[pc.cs_new];
				if(!o)
					k.n_task = task_of_col[size_t(j)];
				REQUIRE(task_of_col[size_t(j)] == k.n_task && pc.linv_off == P.linv_off[j] && pc.cs_src == P.cs_src[j]);
				REQUIRE(pc.slot0 == n_slot && pc.nb == P.lptr[j + 1] - P.lptr[j] && pc.ir0 == n_irow && pc.inr >= 0);
				REQUIRE(o == 0 || pc.sub >= k.cols[size_t(o) - 1].sub); // level by level
				n_level_cols = (o > 0 && pc.sub == k.cols[size_t(o) - 1].sub)? n_level_cols + 1 : 1;
				REQUIRE(n_level_cols <= cfg.n_cap_lvl);
				if(n_level_cols > 1)
					c.reached.insert("tall_tasks");
				for(int q = 0; q < pc.nb; ++ q) {
					k.blk.push_back(P.lptr[j] + q);
					REQUIRE(k.slots[size_t(n_slot + q)].loff == P.loff[P.lptr[j] + q] && k.slots[size_t(n_slot + q)].asrc == R.blks[size_t(P.lptr[j] + q)].asrc);
				}
				n_slot += pc.nb;
				n_irow += pc.inr;
			}
			REQUIRE(n_slot == hd.n_slots && n_irow == hd.n_int_rows);
			REQUIRE(hd.n_cols == P.task_ptr[k.n_task + 1] - P.task_ptr[k.n_task]); // all of the task's columns
			REQUIRE(k.n_task >= P.stage_ptr[s] && k.n_task < P.stage_ptr[s + 1]);
			for(size_t e = 0; e < k.irow.size(); ++ e)
				REQUIRE(int(k.irow[e] & 0xffff) < hd.n_slots && int(k.irow[e] >> 16) < hd.n_cols);
			for(size_t e = 0; e < k.ipair.size(); ++ e)
				REQUIRE(int(k.ipair[e] & 0xffff) < hd.n_slots && int(k.ipair[e] >> 16) < hd.n_slots);
			for(int v = 0; v < cfg.n_waves; ++ v) {
				for(int e = hd.ext_ptr[v]; e < hd.ext_ptr[v + 1]; ++ e) {
					const TPanelExt &en = k.fresh[size_t(e)];
					REQUIRE(int(en.slot) < hd.n_slots && int(en.slot) % cfg.n_waves == v && en.kind <= 3);
					if(en.kind < 2) {
						REQUIRE(en.a_off >= 0 && en.a_off < n_factor && en.b_off >= 0 && en.b_off < n_factor);
						REQUIRE(L.panel_ride[size_t(s)] != 0);
					} else {
						REQUIRE(en.a_off >= 0 && en.a_off + DD + 8 <= R.n_handup_doubles && s > 0);
						c.reached.insert("hand_ups");
					}
					if(en.kind == 1 || en.kind == 3)
						REQUIRE(en.col >= 0 && en.col < hd.n_cols && int(en.slot) == k.cols[size_t(en.col)].slot0);
					if(en.kind == 1)
						REQUIRE(en.ycs >= 0 && en.ycs < n_scalars);
				}
			}
			// its hand-up list
			const int64_t n_out_off = R.panel_out_off[size_t(p)];
			if(n_out_off < 0) {
				REQUIRE(n_out_off == -1 && hd.ext_ptr[10] == 0 && hd.ext_ptr[11] == 0);
				continue;
			}
			const int n_out = hd.ext_ptr[10];
			REQUIRE(n_out >= 1 && hd.ext_ptr[11] <= cfg.n_cap_out && size_t(n_out_off) + size_t(hd.ext_ptr[11]) <= n_pkg_end);
			std::vector<int32_t> level_end;
			REQUIRE(read_units(R.panel_pkg, size_t(n_out_off), 12, level_end));
			for(int l = 0; l < 12; ++ l)
				REQUIRE(level_end[size_t(l)] >= (l? level_end[size_t(l) - 1] : 0) && level_end[size_t(l)] <= n_out);
			REQUIRE(level_end[11] == n_out);
			REQUIRE(read_units(R.panel_pkg, size_t(n_out_off) + 3, size_t(n_out), k.out));
			int n_pairs = 0;
			for(int o = 0; o < n_out; ++ o) {
				REQUIRE(k.out[size_t(o)].op0 == n_pairs && k.out[size_t(o)].onp >= 1);
				n_pairs += k.out[size_t(o)].onp;
				const int64_t n_dst = k.out[size_t(o)].dst & ((int64_t(1) << 62) - 1);
				REQUIRE(n_dst >= 0 && n_dst + DD + 8 <= R.n_handup_doubles && n_dst % (DD + 8) == 0);
			}
			REQUIRE(hd.ext_ptr[11] == 3 + n_out + (n_pairs + 3) / 4);
			REQUIRE(read_units(R.panel_pkg, size_t(n_out_off) + 3 + size_t(n_out), size_t(n_pairs), k.out_pairs));
			for(int o = 0; o < n_out; ++ o) {
				const bool b_diag = (k.out[size_t(o)].dst >> 62) & 1;
				for(int e = k.out[size_t(o)].op0; e < k.out[size_t(o)].op0 + k.out[size_t(o)].onp; ++ e) {
					const uint32_t n_pair = k.out_pairs[size_t(e)];
					REQUIRE(int(n_pair & 0xffff) < hd.n_slots && int(n_pair >> 16) < (b_diag? hd.n_cols : hd.n_slots));
				}
			}
		}
		if(!b_plan_order)
			c.reached.insert("launch_order_sorted");
		if(cfg.b_from_lambda) {
			REQUIRE(L.panel_ride[size_t(s)] == 2);
			if(L.panel_ptr[s + 1] > L.panel_ptr[s])
				c.reached.insert("b_from_lambda_stage");
		}
		if(L.panel_upd_ptr[s + 1] > L.panel_upd_ptr[s] && R.upd_slots[size_t(L.panel_upd_ptr[s + 1]) - 1].e0 + R.upd_slots[size_t(L.panel_upd_ptr[s + 1]) - 1].ne >
		   R.upd_slots[size_t(L.panel_upd_ptr[s])].e0) // (the stage's blocks receive updates through the lists)
			c.reached.insert((L.panel_ride[size_t(s)] == 1)? "riders" : "update_launch");
		if(s == 0 && L.panel_ptr[1] > 0)
			c.reached.insert("leaf_panels");
		REQUIRE(cfg.n_waves == 8 || L.panel_ptr[s + 1] - L.panel_ptr[s] + L.panel_rest_ptr[s + 1] - L.panel_rest_ptr[s] > 0);
		if(cfg.n_waves != 8)
			c.reached.insert(cfg.n_waves == 4? "four_waves" : "two_waves");
	}
	{ // panel_units: the sizes of the packages
		std::multiset<int32_t> a(R.panel_units.begin(), R.panel_units.end()), b;
		for(size_t p = 0; p < pk.size(); ++ p)
			b.insert(pk[p].hd.n_units);
		REQUIRE(a == b);
	}
	// every task of a panel stage is in exactly one package or in panel_rest, and the other stages have neither
	std::vector<int> n_seen(P.task_ptr.size() - 1, 0);
	for(size_t p = 0; p < pk.size(); ++ p)
		++ n_seen[size_t(pk[p].n_task)];
	for(int s = 0; s < n_stages; ++ s) {
		for(int32_t q = L.panel_rest_ptr[s]; q < L.panel_rest_ptr[s + 1]; ++ q) {
			REQUIRE(R.panel_rest[size_t(q)] >= P.stage_ptr[s] && R.panel_rest[size_t(q)] < P.stage_ptr[s + 1]);
			const int t = R.panel_rest[size_t(q)];
			++ n_seen[size_t(t)];
			int64_t n_blocks = 0;
			for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i)
				n_blocks += P.lptr[P.task_cols[i] + 1] - P.lptr[P.task_cols[i]];
			c.reached.insert((P.task_ptr[t + 1] - P.task_ptr[t] > int(PANEL_COLS) || n_blocks > panel_slot_cap(P.max_dim))? "task_over_image" : "task_over_package_units");
		}
		const bool b_panel_stage = s >= c.L.n_bottom_stages || (s == 0 && c.opt.n_simt <= 0 && P.stage_ptr[1] - P.stage_ptr[0] <= 512);
		for(int t = P.stage_ptr[s]; t < P.stage_ptr[s + 1]; ++ t)
			REQUIRE(n_seen[size_t(t)] == (b_panel_stage? 1 : 0));
	}
	return true;
}

// no update lost, none twice: every factor block of a packaged task receives each of the plan's updates exactly once, as
// an internal entry, a fresh entry, an operand pair behind a handed-up block, or an entry of the update lists
static bool check_updates(const char *name, TCase &c, const std::vector<TPackage> &pk)
{
	const Plan &P = c.P;
	const SparseRecords &R = c.R;
	const int64_t n_factor = P.loff.back(), n_scalars = P.cs_new[P.n];
	std::map<int64_t, int64_t> blk_of_loff;
	for(size_t k = 0; k < P.lrow.size(); ++ k)
		blk_of_loff[P.loff[k]] = int64_t(k);
	typedef std::pair<int64_t, int64_t> TOperands; // (block a, block b); row entries: (block, block)
	std::vector<std::multiset<TOperands> > got(P.lrow.size());
	std::vector<int> n_upd_slots(P.lrow.size(), 0);
	// the handed-up blocks: hand-up buffer offset -> the operand pairs behind it, as factor blocks of the source task
	std::map<int64_t, std::vector<TOperands> > handed;
	std::map<int64_t, bool> handed_diag;
	for(size_t p = 0; p < pk.size(); ++ p) {
		const TPackage &k = pk[p];
		for(size_t o = 0; o < k.out.size(); ++ o) {
			const bool b_diag = (k.out[o].dst >> 62) & 1;
			const int64_t n_dst = k.out[o].dst & ((int64_t(1) << 62) - 1);
			REQUIRE(!handed.count(n_dst)); // one record per block of the buffer
			handed_diag[n_dst] = b_diag;
			for(int e = k.out[o].op0; e < k.out[o].op0 + k.out[o].onp; ++ e) {
				const uint32_t n_pair = k.out_pairs[size_t(e)];
				const int64_t ka = k.blk[n_pair & 0xffff];
				if(b_diag) {
					REQUIRE(k.cols[n_pair >> 16].cs_new == P.cs_new[P.blk_col[ka]]); // (the column whose y the product takes)
					handed[n_dst].push_back(TOperands(ka, ka));
				} else
					handed[n_dst].push_back(TOperands(ka, k.blk[n_pair >> 16]));
			}
		}
	}
	size_t n_handed_used = 0;
	for(size_t p = 0; p < pk.size(); ++ p) {
		const TPackage &k = pk[p];
		for(size_t o = 0; o < k.cols.size(); ++ o) { // internal row entries: of the column's diagonal block
			const TPanelCol &pc = k.cols[o];
			for(int e = pc.ir0; e < pc.ir0 + pc.inr; ++ e) {
				const int64_t kb = k.blk[k.irow[size_t(e)] & 0xffff];
				REQUIRE(k.cols[k.irow[size_t(e)] >> 16].cs_new == P.cs_new[P.blk_col[kb]]);
				got[size_t(k.blk[size_t(pc.slot0)])].insert(TOperands(kb, kb));
			}
		}
		for(size_t q = 0; q < k.slots.size(); ++ q) {
			for(int e = k.slots[q].ip0; e < k.slots[q].ip0 + k.slots[q].inp; ++ e)
				got[size_t(k.blk[q])].insert(TOperands(k.blk[k.ipair[size_t(e)] & 0xffff], k.blk[k.ipair[size_t(e)] >> 16]));
		}
		for(size_t e = 0; e < k.fresh.size(); ++ e) {
			const TPanelExt &en = k.fresh[e];
			std::multiset<TOperands> &r_got = got[size_t(k.blk[en.slot])];
			if(en.kind < 2) {
				REQUIRE(blk_of_loff.count(en.a_off) && blk_of_loff.count(en.b_off));
				if(en.kind == 1)
					REQUIRE(en.a_off == en.b_off && en.ycs == P.cs_new[P.blk_col[blk_of_loff[en.a_off]]]);
				r_got.insert(TOperands(blk_of_loff[en.a_off], blk_of_loff[en.b_off]));
			} else {
				REQUIRE(handed.count(en.a_off) && handed_diag[en.a_off] == (en.kind == 3));
				r_got.insert(handed[en.a_off].begin(), handed[en.a_off].end());
				++ n_handed_used;
			}
		}
	}
	REQUIRE(n_handed_used == handed.size() && int64_t(handed.size()) * (P.max_dim * P.max_dim + 8) == R.n_handup_doubles); // every block of the buffer written once, read once
	for(size_t u = 0; u < R.upd_slots.size(); ++ u) {
		const TUpdSlot &us = R.upd_slots[u];
		REQUIRE(blk_of_loff.count(us.loff) && us.e0 >= 0 && us.ne >= 0 && us.e0 + us.ne <= int64_t(R.upd_ents.size()));
		const int64_t k = blk_of_loff[us.loff];
		const bool b_diag = k == P.lptr[P.blk_col[k]];
		REQUIRE(us.kind == (b_diag? 1 : 0) && us.asrc == R.blks[size_t(k)].asrc);
		if(b_diag)
			REQUIRE(us.cs_new == P.cs_new[P.blk_col[k]] && us.cs_src == P.cs_src[P.blk_col[k]]);
		++ n_upd_slots[size_t(k)];
		for(int64_t e = us.e0; e < us.e0 + us.ne; ++ e) {
			const TUpdEnt &en = R.upd_ents[size_t(e)];
			REQUIRE(en.a_off >= 0 && en.a_off < n_factor && blk_of_loff.count(en.a_off));
			if(b_diag) {
				REQUIRE(en.b_off >= 0 && en.b_off < n_scalars && en.b_off == P.cs_new[P.blk_col[blk_of_loff[en.a_off]]]);
				got[size_t(k)].insert(TOperands(blk_of_loff[en.a_off], blk_of_loff[en.a_off]));
			} else {
				REQUIRE(en.b_off >= 0 && en.b_off < n_factor && blk_of_loff.count(en.b_off));
				got[size_t(k)].insert(TOperands(blk_of_loff[en.a_off], blk_of_loff[en.b_off]));
			}
		}
	}
	std::vector<char> packaged(P.lrow.size(), 0);
	for(size_t p = 0; p < pk.size(); ++ p) {
		for(size_t q = 0; q < pk[p].blk.size(); ++ q) {
			const int64_t k = pk[p].blk[q];
			const int32_t j = P.blk_col[k];
			REQUIRE(!packaged[size_t(k)]);
			packaged[size_t(k)] = 1;
			std::multiset<TOperands> want;
			if(k == P.lptr[j]) {
				for(int64_t e = P.rptr[j]; e < P.rptr[j + 1]; ++ e)
					want.insert(TOperands(P.rblk[e], P.rblk[e]));
				REQUIRE(int64_t(got[size_t(k)].size()) == P.rptr[j + 1] - P.rptr[j]);
			} else {
				for(int64_t e = P.pptr[k]; e < P.pptr[k + 1]; ++ e)
					want.insert(TOperands(P.pa[e], P.pb[e]));
				REQUIRE(int64_t(got[size_t(k)].size()) == P.pptr[k + 1] - P.pptr[k]);
			}
			REQUIRE(got[size_t(k)] == want);
			REQUIRE(n_upd_slots[size_t(k)] == 1);
		}
	}
	for(size_t k = 0; k < P.lrow.size(); ++ k)
		REQUIRE(packaged[k] || (got[k].empty() && !n_upd_slots[k]));
	return true;
}

static bool check_dense_top(const char *name, TCase &c)
{
	const Plan &P = c.P;
	const SparseRecords &R = c.R;
	if(!P.dense_dim) {
		REQUIRE(R.dense_blks.empty() && R.dense_cols.empty() && R.dense_blk_loff.empty() && R.gaps.empty() && R.unit.empty() && R.dst.empty());
		return true;
	}
	c.reached.insert("dense_top");
	const int n_pad = (P.dense_dim + 1 + 63) / 64 * 64;
	const int64_t n_scalars = P.cs_new[P.n];
	REQUIRE(R.dense_blks.size() == R.dense_blk_loff.size() && int(R.unit.size()) == n_pad && int(R.dst.size()) == n_pad);
	std::vector<int> n_covered(size_t(n_pad), 0);
	for(size_t k = 0; k < R.dense_cols.size(); ++ k) {
		const TDenseCol &dc = R.dense_cols[k];
		REQUIRE(dc.pos >= 0 && dc.pos + dc.dj <= P.dense_dim && dc.cs_new + dc.dj <= n_scalars && dc.cs_src + dc.dj <= n_scalars);
		for(int q = 0; q < dc.dj; ++ q) {
			++ n_covered[size_t(dc.pos + q)];
			REQUIRE(R.unit[size_t(dc.pos + q)] == 0 && R.dst[size_t(dc.pos + q)].x == dc.cs_new + q && R.dst[size_t(dc.pos + q)].y == dc.cs_src + q);
		}
	}
	size_t n_gap = 0;
	for(int q = 0; q < n_pad; ++ q) {
		REQUIRE(n_covered[size_t(q)] <= 1);
		if(n_covered[size_t(q)])
			continue;
		REQUIRE(R.unit[size_t(q)] == 1 && R.dst[size_t(q)].x == -1 && R.dst[size_t(q)].y == -1);
		if(q < P.dense_dim) {
			REQUIRE(n_gap < R.gaps.size() && R.gaps[n_gap] == q);
			++ n_gap;
		}
	}
	REQUIRE(n_gap == R.gaps.size());
	if(n_gap)
		c.reached.insert("dense_gaps");
	for(size_t k = 0; k < R.dense_blks.size(); ++ k) {
		const TDenseBlk &b = R.dense_blks[k];
		REQUIRE(b.dst >= 0 && b.dst % n_pad + b.di <= P.dense_dim && b.dst / n_pad + b.dj <= P.dense_dim);
		REQUIRE(b.p0 >= 0 && b.np >= 0 && b.p0 + b.np <= int64_t(P.pa.size()));
		REQUIRE(b.nr == -1 || (b.r0 >= 0 && b.r0 + b.nr <= int64_t(P.rblk.size()) && b.cs_src + b.dj <= n_scalars && b.pos + b.dj <= P.dense_dim));
		REQUIRE(R.dense_blk_loff[k] >= 0 && R.dense_blk_loff[k] + int64_t(b.di) * b.dj <= P.loff.back());
	}
	return true;
}

// lane-per-task tables: every task of a stage in exactly one chunk or in the rest list, and every table entry of a lane
// the offset its own task's program means by it
static bool check_simt(const char *name, TCase &c)
{
	const Plan &P = c.P;
	const SparseRecords &R = c.R;
	const SparseLaunchLists &L = c.L;
	if(L.simt_chunk_ptr.empty()) {
		REQUIRE(R.simt_chunks.empty() && L.simt_rest_ptr.empty());
		return true;
	}
	c.reached.insert("lane_per_task");
	const size_t W = size_t(c.opt.n_simt_width);
	const int n_used = int(L.simt_chunk_ptr.size()) - 1;
	REQUIRE(int(L.simt_rest_ptr.size()) == n_used + 1 && int(L.simt_lds_bytes.size()) == n_used && int(L.simt_bwd_lds_bytes.size()) == n_used);
	REQUIRE(L.simt_chunk_ptr.back() == int32_t(R.simt_chunks.size()) && L.simt_rest_ptr.back() == int32_t(R.simt_rest.size()));
	REQUIRE(R.simt_chunks.size() == R.simt_bwd_chunks.size());
	std::map<int64_t, int32_t> col_of_loff; // offset of a column's diagonal block -> column
	std::vector<int32_t> task_of_col(size_t(P.n), -1);
	for(int32_t j = 0; j < P.n; ++ j)
		col_of_loff[P.loff[P.lptr[j]]] = j;
	for(int t = 0; t + 1 < int(P.task_ptr.size()); ++ t) {
		for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i)
			task_of_col[P.task_cols[i]] = t;
	}
	std::vector<int> n_seen(P.task_ptr.size() - 1, 0);
	for(int s = 0; s < n_used; ++ s) {
		REQUIRE(L.simt_chunk_ptr[s] <= L.simt_chunk_ptr[s + 1] && L.simt_rest_ptr[s] <= L.simt_rest_ptr[s + 1]);
		for(int32_t q = L.simt_rest_ptr[s]; q < L.simt_rest_ptr[s + 1]; ++ q) {
			REQUIRE(R.simt_rest[size_t(q)] >= P.stage_ptr[s] && R.simt_rest[size_t(q)] < P.stage_ptr[s + 1]);
			++ n_seen[size_t(R.simt_rest[size_t(q)])];
			c.reached.insert("lane_per_task_rest");
		}
		for(int32_t n_chunk = L.simt_chunk_ptr[s]; n_chunk < L.simt_chunk_ptr[s + 1]; ++ n_chunk) {
			const TSimtChunk &ch = R.simt_chunks[size_t(n_chunk)], &bw = R.simt_bwd_chunks[size_t(n_chunk)];
			REQUIRE(ch.n_tasks >= 1 && ch.n_tasks <= int(W) && bw.n_tasks == ch.n_tasks);
			REQUIRE(ch.prog_off >= 0 && size_t(ch.prog_off) + 4 <= R.simt_prog.size());
			const int32_t *prog = &R.simt_prog[size_t(ch.prog_off)];
			const int n_cols = prog[0], n_blocks = prog[1], n_ops = prog[2], n_ys = prog[3];
			const int n_fields = 4 * n_cols + n_blocks + n_ops + n_ys, n_bwd_fields = 3 * n_cols + (n_blocks - n_cols);
			REQUIRE(ch.tab_off >= 0 && size_t(ch.tab_off) + size_t(n_fields) * W <= R.simt_tab.size() && n_fields * int(W) * 8 <= L.simt_lds_bytes[size_t(s)]);
			REQUIRE(bw.tab_off >= 0 && size_t(bw.tab_off) + size_t(n_bwd_fields) * W <= R.simt_bwd_tab.size());
			REQUIRE((n_bwd_fields + n_cols * P.max_dim) * int(W) * 8 <= L.simt_bwd_lds_bytes[size_t(s)]);
			REQUIRE(bw.prog_off >= 0 && size_t(bw.prog_off) + 2 + size_t(n_cols) + size_t(n_blocks - n_cols) <= R.simt_bwd_prog.size());
			const int32_t *bprog = &R.simt_bwd_prog[size_t(bw.prog_off)];
			REQUIRE(bprog[0] == n_cols && bprog[1] == n_blocks - n_cols);
			const int64_t *tab = &R.simt_tab[size_t(ch.tab_off)], *btab = &R.simt_bwd_tab[size_t(bw.tab_off)];
			for(int n_lane = 0; n_lane < int(W); ++ n_lane) {
				auto T = [&](int f) { return tab[size_t(f) * W + size_t(n_lane)]; };
				auto B = [&](int f) { return btab[size_t(f) * W + size_t(n_lane)]; };
				REQUIRE(col_of_loff.count(T(0)));
				const int t = task_of_col[size_t(col_of_loff[T(0)])];
				REQUIRE(t >= P.stage_ptr[s] && t < P.stage_ptr[s + 1] && P.task_ptr[t + 1] - P.task_ptr[t] == n_cols);
				if(n_lane < ch.n_tasks)
					++ n_seen[size_t(t)];
				else
					REQUIRE(T(0) == tab[size_t(ch.n_tasks) - 1]); // spare lanes repeat the last task
				// walk the program with this lane's table: every operand and y it names must be this task's
				const int f_blk = 4 * n_cols, f_op = f_blk + n_blocks, f_y = f_op + n_ops;
				size_t n_at = 4, n_blk_at = 0;
				int f_bwd = 3 * n_cols, n_sub = 0;
				for(int o = 0; o < n_cols; ++ o) {
					const int32_t j = P.task_cols[size_t(P.task_ptr[t]) + size_t(o)];
					REQUIRE(T(4 * o) == P.loff[P.lptr[j]] && T(4 * o + 1) == P.linv_off[j] && T(4 * o + 2) == P.cs_new[j] && T(4 * o + 3) == P.cs_src[j]);
					REQUIRE(B(3 * o) == P.loff[P.lptr[j]] && B(3 * o + 1) == P.cs_new[j] && B(3 * o + 2) == P.cs_src[j]);
					REQUIRE(size_t(ch.prog_off) + n_at + 3 <= R.simt_prog.size());
					const int nb = prog[n_at], nr = prog[n_at + 1], n_touch = prog[n_at + 2];
					REQUIRE(nb == P.lptr[j + 1] - P.lptr[j] && nr == P.rptr[j + 1] - P.rptr[j] && bprog[2 + o] == nb);
					n_at += 3;
					for(int q = 0; q < n_touch; ++ q)
						REQUIRE(prog[n_at + size_t(q)] >= 0 && prog[n_at + size_t(q)] < n_ops);
					n_at += size_t(n_touch);
					for(int q = 0; q < nb; ++ q, ++ n_blk_at) {
						const int64_t k = P.lptr[j] + q;
						REQUIRE(T(f_blk + int(n_blk_at)) == ((P.asrc[k] < 0)? -1 : P.asrc[k] * 2 + P.atrans[k]));
					}
					for(int e = 0; e < nr; ++ e, n_at += 2) {
						const int32_t n_blk = P.rblk[P.rptr[j] + e];
						REQUIRE(prog[n_at] >= 0 && prog[n_at] < n_ops && prog[n_at + 1] >= 0 && prog[n_at + 1] < n_ys);
						REQUIRE(T(f_op + prog[n_at]) == P.loff[n_blk] && T(f_y + prog[n_at + 1]) == P.cs_new[P.blk_col[n_blk]]);
					}
					for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k, ++ n_sub) {
						REQUIRE(prog[n_at] == P.pptr[k + 1] - P.pptr[k]);
						++ n_at;
						for(int64_t e = P.pptr[k]; e < P.pptr[k + 1]; ++ e, n_at += 2) {
							REQUIRE(prog[n_at] >= 0 && prog[n_at] < n_ops && prog[n_at + 1] >= 0 && prog[n_at + 1] < n_ops);
							REQUIRE(T(f_op + prog[n_at]) == P.loff[P.pa[e]] && T(f_op + prog[n_at + 1]) == P.loff[P.pb[e]]);
						}
						REQUIRE(B(f_bwd + n_sub) == P.cs_new[P.lrow[k]]);
					}
				}
				REQUIRE(int(n_blk_at) == n_blocks && n_sub == n_blocks - n_cols);
			}
		}
		for(int t = P.stage_ptr[s]; t < P.stage_ptr[s + 1]; ++ t)
			REQUIRE(n_seen[size_t(t)] == 1);
	}
	return true;
}

static PlanOptions variant_plan_options() // ~n/4 leaf tasks, six or more stages, no dense top (tests/variant_util.py)
{
	PlanOptions opt;
	opt.subtree_size = 4;
	opt.leaf_size = 1;
	opt.dense_top_nb = 0;
	return opt;
}

static SparseRecordOptions default_record_options()
{
	SparseRecordOptions t_opt = {-1, 1, -1, 32, 1, 8192, true, false};
	return t_opt;
}

static bool run(const char *name, int n, const CEdgeList &edges, const std::vector<int> &dims, PlanOptions plan_opt,
	const SparseRecordOptions &rec_opt)
{
	TCase c;
	c.opt = rec_opt;
	// (what the analysis sets before it plans: the panel kernel's capacities)
	plan_opt.task_wide_min = std::max(rec_opt.n_wide_min_tasks, 1);
	plan_opt.task_max_cols = int(PANEL_COLS);
	plan_opt.task_max_blocks = panel_slot_cap(dims[0]);
	if(!plan_of_graph(name, n, edges, dims, plan_opt, c.P))
		return false;
	build_all(c);
	std::vector<TPackage> pk;
	if(!check_column_records(name, c) || !check_column_packages(name, c) || !decode_packages(name, c, pk) || !check_updates(name, c, pk) ||
	   !check_dense_top(name, c) || !check_simt(name, c))
		return false;
	printf("%s: columns %d stages %d packages %zu reached", name, c.P.n, int(c.P.stage_ptr.size()) - 1, pk.size());
	for(std::set<std::string>::const_iterator p = c.reached.begin(); p != c.reached.end(); ++ p)
		printf(" %s", p->c_str());
	printf(" ok\n");
	return true;
}

static void set_knob(const char *p_s_name, const char *p_s_value)
{
	if(p_s_value)
		setenv(p_s_name, p_s_value, 1);
	else
		unsetenv(p_s_name);
}

int main()
{
	setenv("SLAMPP_HIP_DEV", "1", 1); // (the development knobs below are read only with it: plan.h)
	dev_knobs_refresh();
	std::mt19937 rng(7);
	bool b_ok = true;
	const std::vector<int> d6(1, 6), d3(1, 3), d7(1, 7);
	const CEdgeList chain = chain_with_closures(612, rng);
	{ // the schedule of a large graph at 600 poses: wide stages, crowded slice launches
		SparseRecordOptions t_opt = default_record_options();
		t_opt.n_wide_min_tasks = 8;
		set_knob("SLAMPP_HIP_DEV_PANEL_W4_MIN", "0");
		set_knob("SLAMPP_HIP_DEV_PANEL_W2_MIN", "0");
		b_ok = run("chain6", 612, chain, d6, variant_plan_options(), t_opt) && b_ok;
		set_knob("SLAMPP_HIP_DEV_PANEL_RIDE_FRESH", "0");
		b_ok = run("chain6-no-riders", 612, chain, d6, variant_plan_options(), t_opt) && b_ok;
		set_knob("SLAMPP_HIP_DEV_PANEL_RIDE_FRESH", 0);
		t_opt.n_panel_handup = 0;
		b_ok = run("chain6-no-hand-ups", 612, chain, d6, variant_plan_options(), t_opt) && b_ok;
		t_opt.n_panel_handup = 1;
		set_knob("SLAMPP_HIP_DEV_PANEL_W2_MIN", 0);
		b_ok = run("chain6-four-waves", 612, chain, d6, variant_plan_options(), t_opt) && b_ok;
		set_knob("SLAMPP_HIP_DEV_PANEL_W4_MIN", 0);
		t_opt.n_simt = 1;
		const int widths[] = {16, 32, 64};
		for(int w = 0; w < 3; ++ w) {
			t_opt.n_simt_width = widths[w];
			t_opt.n_simt_stages = (w == 0)? 3 : 1;
			t_opt.n_wide_min_tasks = (w == 0)? 8 : 8192; // (32, 64: the first slice stage sits right on the lane-per-task leaves)
			b_ok = run((std::string("chain6-lanes") + std::to_string(widths[w])).c_str(), 612, chain, d6, variant_plan_options(), t_opt) && b_ok;
		}
		t_opt = default_record_options();
		t_opt.n_simt = 0; // at most 512 leaf tasks: leaf panels
		b_ok = run("chain6-leaf-panels", 612, chain, d6, variant_plan_options(), t_opt) && b_ok;
		b_ok = run("chain3", 612, chain, d3, variant_plan_options(), t_opt) && b_ok; // slot caps 256 and 72
		b_ok = run("chain7", 612, chain, d7, variant_plan_options(), t_opt) && b_ok;
		const int mixed[] = {2, 3, 6, 7, 8, 4, 5};
		b_ok = run("mixed", 612, chain, std::vector<int>(mixed, mixed + 7), variant_plan_options(), default_record_options()) && b_ok;
	}
	{ // more than 512 leaf tasks on a system that is not small: the records of the separator stages first
		const CEdgeList e = chain_with_closures(3000, rng);
		SparseRecordOptions t_opt = default_record_options();
		t_opt.b_small = false;
		t_opt.n_wide_min_tasks = 64;
		b_ok = run("chain6-3000", 3000, e, d6, variant_plan_options(), t_opt) && b_ok;
	}
	{ // a hub: columns over the limits of the column packages, tasks over those of the panel packages
		const int n = 300;
		CEdgeList e = chain_with_closures(n, rng);
		for(int i = 10; i < 130; ++ i)
			e.push_back(std::make_pair(i, n)); // the hub, vertex n
		for(int i = 180; i < 260; ++ i) { // a banded stretch
			e.push_back(std::make_pair(i, i + 2));
			e.push_back(std::make_pair(i, i + 3));
		}
		const int n_clique = 110; // its first columns have more blocks than an image has slots (96 and 72)
		for(int i = 0; i < n_clique; ++ i) {
			e.push_back(std::make_pair(150, n + 1 + i));
			for(int k = 0; k < i; ++ k)
				e.push_back(std::make_pair(n + 1 + k, n + 1 + i));
		}
		SparseRecordOptions t_opt = default_record_options();
		t_opt.n_wide_min_tasks = 1;
		b_ok = run("hub", n + 1 + n_clique, e, d6, variant_plan_options(), t_opt) && b_ok;
		t_opt.n_wide_min_tasks = 8;
		b_ok = run("hub-wide8", n + 1 + n_clique, e, d6, variant_plan_options(), t_opt) && b_ok;
		t_opt.n_simt = 0;
		b_ok = run("hub7-leaf-panels", n + 1 + n_clique, e, d7, variant_plan_options(), t_opt) && b_ok;
	}
	{ // a star: the centre's task rides and brings in one update per leaf task, more than a package holds
		const int n = 512;
		CEdgeList e;
		for(int i = 0; i < n; ++ i)
			e.push_back(std::make_pair(i, n));
		SparseRecordOptions t_opt = default_record_options();
		t_opt.n_simt = 0;
		set_knob("SLAMPP_HIP_DEV_PANEL_RIDE_FRESH", "100000");
		b_ok = run("star", n + 1, e, d6, variant_plan_options(), t_opt) && b_ok;
		set_knob("SLAMPP_HIP_DEV_PANEL_RIDE_FRESH", 0);
	}
	{ // a grid with a forced dense top ...
		PlanOptions opt;
		opt.dense_top_nb = 4;
		opt.dense_top_auto = false;
		opt.dense_top_min_dim = 0;
		b_ok = run("grid+dense_top", 20 * 20, grid_graph(20), d3, opt, default_record_options()) && b_ok;
		// ... and two chains in the caller's order that meet in a last vertex, all of it dense top: each chain is at least a
		// tile long, so the second starts at a tile boundary and leaves a gap behind the first
		CEdgeList e;
		for(int i = 0; i < 30; ++ i) {
			e.push_back(std::make_pair(i, (i + 1 < 30)? i + 1 : 60));
			e.push_back(std::make_pair(30 + i, (i + 1 < 30)? 30 + i + 1 : 60));
		}
		opt.dense_top_nb = 2;
		opt.natural_order = true;
		b_ok = run("two-chains+dense_top", 61, e, d3, opt, default_record_options()) && b_ok;
	}
	return b_ok? 0 : 1;
}
