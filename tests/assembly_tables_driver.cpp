// assembly_tables_driver.cpp -- the host builder of the Lambda / eta assembly (csrc/assembly_tables.cpp) on the CPU, for
// tests/test_assembly_tables_sanitizers.py and tests/test_assembly_routes_gpu.py.
//   driver <cases file>   every case of the file (tests/assembly_cases.py: case_text): builds Lambda's structure from the
//                         dimensions, the edges and the extra pairs, runs the builder, decodes every table the way the
//                         kernel that reads it does (assembly.hip) and checks it against a brute-force walk of the edges;
//                         prints one line per case: the counts of slampp_hip_assembly_get_info, every vertex's route
//                         (G group, L long, S packed, P one wave) and the branches reached, " ok" at its end if all held
//   driver refusals       what the builder must refuse
//   driver sweep          asm_group_shape() over rd <= 8, d0, d1 <= 7: the group kernel's instantiations that can be reached
#include "assembly_tables.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <stdexcept>
#include <string>

using namespace slampp;

static int n_failures = 0;
#define CHECK(c) do { if(!(c)) { if(n_failures < 50) fprintf(stderr, "failed at line %d: %s\n", __LINE__, #c); ++ n_failures; } } while(0)

struct TCase {
	std::string name;
	int64_t n, n_edges;
	int rd, n_groups_option;
	std::vector<int64_t> dims, v0, v1, cs, ptr;
	std::vector<int32_t> brow;
};

static void Build_Structure(TCase &c, const std::vector<int64_t> &extra)
{
	std::set<std::pair<int64_t, int64_t> > blocks; // (column, row)
	for(int64_t v = 0; v < c.n; ++ v)
		blocks.insert(std::make_pair(v, v));
	for(int64_t e = 0; e < c.n_edges; ++ e)
		blocks.insert(std::make_pair(std::max(c.v0[e], c.v1[e]), std::min(c.v0[e], c.v1[e])));
	for(size_t i = 0; i + 1 < extra.size(); i += 2)
		blocks.insert(std::make_pair(std::max(extra[i], extra[i + 1]), std::min(extra[i], extra[i + 1])));
	c.cs.assign(1, 0);
	for(int64_t v = 0; v < c.n; ++ v)
		c.cs.push_back(c.cs.back() + c.dims[v]);
	c.ptr.assign(c.n + 1, 0);
	c.brow.clear();
	for(const auto &b : blocks) {
		++ c.ptr[b.first + 1];
		c.brow.push_back(int32_t(b.second));
	}
	for(int64_t v = 0; v < c.n; ++ v)
		c.ptr[v + 1] += c.ptr[v];
}

static int effective_groups(int n_option) { return (n_option < 0)? 1 << 20 : n_option; } // (the solver's default)

static void Run_Case(TCase &c)
{
	const int n_fail_before = n_failures;
	const int64_t n = c.n, n_edges = c.n_edges;
	const int64_t *cs = c.cs.data(), *ptr = c.ptr.data();
	const int32_t *brow = c.brow.data();
	const int n_option = effective_groups(c.n_groups_option);
	TAsmTables t;
	assembly_build_tables(t, n, cs, ptr, brow, n_edges, c.v0.data(), c.v1.data(), c.rd, n_option);
	const int rd = c.rd, d0 = int(c.dims[c.v0[0]]), d1 = int(c.dims[c.v1[0]]);
	CHECK(t.rd == rd && t.d0 == d0 && t.d1 == d1);
	std::set<std::string> reached;
	// brute force: the value offset of every block, and the list of every block in edge order
	const int64_t n_blocks = ptr[n];
	std::vector<int64_t> voff(n_blocks + 1, 0), col_of(n_blocks);
	std::map<int64_t, int64_t> blk_at; // value offset -> block
	for(int64_t v = 0; v < n; ++ v) {
		for(int64_t k = ptr[v]; k < ptr[v + 1]; ++ k) {
			voff[k + 1] = voff[k] + c.dims[brow[k]] * c.dims[v];
			col_of[k] = v;
			blk_at[voff[k]] = k;
		}
	}
	std::vector<std::vector<int32_t> > want(n_blocks);
	std::vector<int64_t> n_v_edges(n, 0);
	for(int64_t e = 0; e < n_edges; ++ e) {
		const int64_t r = std::min(c.v0[e], c.v1[e]), q = std::max(c.v0[e], c.v1[e]);
		int64_t k = ptr[q];
		while(k < ptr[q + 1] && brow[k] != r)
			++ k;
		CHECK(k < ptr[q + 1]);
		want[k].push_back(int32_t(e * 2 + (c.v0[e] > c.v1[e])));
		want[ptr[c.v0[e] + 1] - 1].push_back(int32_t(e * 2));
		want[ptr[c.v1[e] + 1] - 1].push_back(int32_t(e * 2 + 1));
		++ n_v_edges[c.v0[e]]; ++ n_v_edges[c.v1[e]];
		if(c.v0[e] > c.v1[e])
			reached.insert("flipped_edge");
	}
	for(int64_t k = 0; k < n_blocks; ++ k) {
		if(brow[k] != col_of[k] && want[k].empty()) reached.insert("edgeless_block");
		if(brow[k] != col_of[k] && want[k].size() > 1) reached.insert("multi_edge_block");
		if(brow[k] == col_of[k] && want[k].empty()) reached.insert("edgeless_vertex");
	}
	std::vector<int> n_block_writes(n_blocks, 0), n_eta_writes(n, 0);
	std::string routes(size_t(n), '?');
	// the edge planes of linearize.hip
	CHECK(int64_t(t.edge_state.size()) == 3 * n_edges);
	for(int64_t e = 0; e < n_edges && t.edge_state.size() == size_t(3 * n_edges); ++ e)
		CHECK(t.edge_state[e] == cs[c.v0[e]] && t.edge_state[n_edges + e] == cs[c.v1[e]] && t.edge_state[2 * n_edges + e] == c.v0[e]);
	// a record of the one-wave, the packed and the edge-parallel kernels: its block, its list
	auto Check_Record = [&](const TAsmBlk &b, bool b_diag, int64_t n_vertex) -> int64_t {
		auto it = blk_at.find(b.dst);
		CHECK(it != blk_at.end());
		if(it == blk_at.end())
			return -1;
		const int64_t k = it->second, v = col_of[k];
		CHECK((brow[k] == v) == b_diag);
		CHECK(b.rows == c.dims[brow[k]] && b.cols == c.dims[v]);
		CHECK(b.ne == int64_t(want[k].size()));
		if(b_diag) {
			CHECK(v == n_vertex && b.eta_off == cs[v]);
			++ n_eta_writes[v];
		}
		++ n_block_writes[k];
		if(b.ne != int64_t(want[k].size()))
			return k;
		if(!b_diag && b.ne == 1) { // assemble_offdiag_kernel: ent = (bd.ne == 1)? int32_t(bd.e0) : entries[bd.e0 + i]
			CHECK(int32_t(b.e0) == want[k][0]);
			reached.insert("single_entry_record");
		} else {
			CHECK(b.e0 >= 0 && b.e0 + b.ne <= int64_t(t.entries.size()));
			for(int64_t i = 0; i < b.ne && b.e0 >= 0 && b.e0 + b.ne <= int64_t(t.entries.size()); ++ i)
				CHECK(t.entries[b.e0 + i] == want[k][i]);
		}
		return k;
	};
	// groups, as assemble_group_kernel reads a package
	const TAsmGroupShape t_shape = asm_group_shape(rd, d0, d1);
	const int n_cap = 4 * t_shape.n_ew;
	CHECK(t.n_grp_cap_edges == n_cap);
	if(n_option == 0)
		reached.insert("groups_off");
	else if(n_cap < 8)
		reached.insert("no_groups_cap_under_8");
	if(n_option == 0 || n_cap < 8)
		CHECK(t.n_groups == 0);
	if(t.n_groups) {
		char p_s_name[32];
		snprintf(p_s_name, sizeof(p_s_name), "group_kernel_%d", (rd == 2 || rd == 3 || rd == 6 || rd == 7)? rd : 0);
		reached.insert(p_s_name);
		CHECK(t.n_grp_pkg_stride % 4 == 0 && t.n_grp_pkg_stride <= GRP_PACKAGE_WORDS);
		CHECK(int64_t(t.grp_words.size()) == t.n_groups * t.n_grp_pkg_stride);
		CHECK(size_t(t.n_grp_pkg_stride) * 4 + size_t(n_cap) * t_shape.n_edge_bytes + 72 * 8 <= 64 * 1024); // the launch's LDS: what a workgroup may ask for (six to a CU while the package stays small)
		CHECK(size_t(n_cap) * t_shape.n_edge_bytes <= GRP_LDS_BYTES);
		CHECK(t.n_grp_pkg_stride <= 256 * GRP_PKG_PER_THREAD); // (the package goes through PKW registers of 256 lanes)
	}
	std::vector<int64_t> grp_first(t.n_groups, -1), grp_last(t.n_groups, -1), grp_words_used(t.n_groups, 0);
	std::vector<std::set<int32_t> > grp_edges(t.n_groups);
	int n_max_stride = 0;
	for(int64_t g = 0; g < t.n_groups && int64_t(t.grp_words.size()) == t.n_groups * t.n_grp_pkg_stride; ++ g) {
		const int32_t *p = t.grp_words.data() + g * t.n_grp_pkg_stride;
		const int n_e = p[0], n_b = p[1], n_ent = p[2], n_items = p[3];
		CHECK(n_e >= 0 && n_e <= n_cap && n_b > 0 && n_ent >= 0 && n_items > 0);
		const int n_words = 4 + n_cap + 6 * n_b + n_ent + (n_items + 1) / 2;
		CHECK(n_words <= t.n_grp_pkg_stride && n_words <= GRP_PACKAGE_WORDS);
		if(n_words > t.n_grp_pkg_stride)
			continue;
		n_max_stride = std::max(n_max_stride, n_words);
		if(!n_e)
			reached.insert("empty_group_package");
		for(int i = 0; i < n_cap; ++ i) // (the kernel requests every slot, padding included)
			CHECK(p[4 + i] >= 0 && p[4 + i] < n_edges);
		for(int i = 0; i < n_e; ++ i)
			CHECK(grp_edges[g].insert(p[4 + i]).second);
		const int32_t *p_blk = p + 4 + n_cap, *p_ent = p_blk + 6 * n_b;
		const uint16_t *p_item = reinterpret_cast<const uint16_t*>(p_ent + n_ent);
		std::vector<int> n_cols_want(n_b, 0), n_list(n_b, 0);
		int n_items_want = 0;
		for(int b = 0; b < n_b; ++ b) {
			const int64_t dst = int64_t(uint64_t(uint32_t(p_blk[6 * b])) | (uint64_t(uint32_t(p_blk[6 * b + 1])) << 32));
			const int eta_off = p_blk[6 * b + 2], v = p_blk[6 * b + 3], n_begin = p_blk[6 * b + 4] & 0xffff, ne = int(uint32_t(p_blk[6 * b + 4]) >> 16);
			const int rows = p_blk[6 * b + 5] & 0xff, cols = (p_blk[6 * b + 5] >> 8) & 0xff;
			auto it = blk_at.find(dst);
			CHECK(it != blk_at.end() && v >= 0 && v < n);
			if(it == blk_at.end() || v < 0 || v >= n)
				continue;
			const int64_t k = it->second;
			const bool b_diag = brow[k] == v;
			CHECK(col_of[k] == v && (eta_off >= 0) == b_diag && (!b_diag || eta_off == cs[v]));
			CHECK(rows == c.dims[brow[k]] && cols == c.dims[v]);
			CHECK(int64_t(want[k].size()) < 32768 && ne == int(want[k].size())); // (n_begin | ne << 16 in an int32_t)
			CHECK(n_begin + ne <= n_ent && n_ent < 65536);
			for(int i = 0; i < ne && ne == int(want[k].size()) && n_begin + ne <= n_ent; ++ i) {
				const int32_t ent = p_ent[n_begin + i];
				CHECK(ent >= 0 && (ent >> 1) < n_cap && (ent >> 1) < n_e);
				if(ent >= 0 && (ent >> 1) < n_e)
					CHECK(p[4 + (ent >> 1)] * 2 + (ent & 1) == want[k][i]);
			}
			++ n_block_writes[k];
			n_cols_want[b] = cols + (b_diag? 1 : 0);
			n_list[b] = ne;
			n_items_want += n_cols_want[b];
			if(b_diag) {
				routes[v] = 'G';
				CHECK(n_v_edges[v] <= n_cap);
				grp_first[g] = (grp_first[g] < 0)? v : std::min(grp_first[g], int64_t(v));
				grp_last[g] = std::max(grp_last[g], int64_t(v));
				grp_words_used[g] += (6 + 4) * (ptr[v + 1] - ptr[v]) + 3 * n_v_edges[v] + 1;
			}
		}
		CHECK(n_items == n_items_want);
		std::set<int> items_seen;
		int n_prev_len = -1;
		for(int i = 0; i < n_items; ++ i) {
			const int n_code = p_item[i], b = n_code >> 3, q = n_code & 7;
			CHECK(b < n_b && q < ((b < n_b)? n_cols_want[b] : 0));
			CHECK(items_seen.insert(n_code).second);
			if(b < n_b) {
				CHECK(n_list[b] >= n_prev_len); // sorted by list length
				n_prev_len = n_list[b];
				if(q == n_cols_want[b] - 1 && p_blk[6 * b + 2] >= 0)
					++ n_eta_writes[p_blk[6 * b + 3]]; // column `cols` of a diagonal block: eta
			}
		}
	}
	if(t.n_groups)
		CHECK(((n_max_stride + 3) & ~3) == t.n_grp_pkg_stride);
	// a group holds consecutive vertices, all blocks of their columns, and closed for a reason
	auto Vertex_Words = [&](int64_t v) { return (6 + 4) * (ptr[v + 1] - ptr[v]) + 3 * n_v_edges[v] + 1; };
	for(int64_t g = 0; g < t.n_groups; ++ g) {
		CHECK(grp_first[g] >= 0);
		if(grp_first[g] < 0)
			continue;
		CHECK(grp_last[g] - grp_first[g] + 1 <= n_option);
		for(int64_t v = grp_first[g]; v <= grp_last[g]; ++ v)
			CHECK(routes[v] == 'G');
		if(g)
			CHECK(grp_first[g] > grp_last[g - 1]);
		const int64_t v = grp_last[g] + 1;
		if(v == n)
			continue;
		const bool b_next_grouped = g + 1 < t.n_groups && grp_first[g + 1] == v;
		if(!b_next_grouped) {
			const bool b_over_cap = n_v_edges[v] > n_cap, b_over_pkg = Vertex_Words(v) + 4 + n_cap > GRP_PACKAGE_WORDS;
			CHECK(b_over_cap || b_over_pkg);
			if(b_over_cap) reached.insert("vertex_over_cap_closes_group");
			if(b_over_pkg) reached.insert("vertex_over_package_closes_group");
		} else {
			std::set<int32_t> t_union(grp_edges[g]);
			for(int32_t ent : want[ptr[v + 1] - 1])
				t_union.insert(ent >> 1);
			if(grp_last[g] - grp_first[g] + 1 == n_option)
				reached.insert("group_closed_at_vertex_count");
			else if(int(t_union.size()) > n_cap)
				reached.insert("group_closed_at_edge_cap");
			else if(grp_words_used[g] + Vertex_Words(v) + 4 + n_cap > GRP_PACKAGE_WORDS)
				reached.insert("group_closed_at_package_words");
			else
				CHECK(!"a group closed before the next vertex, which would have fit");
		}
	}
	// the other kernels
	const bool b_can_pack = rd == 2 || rd == 3;
	CHECK(t.long_blks.size() == t.long_vertex.size() && t.small_blks.size() == t.small_vertex.size() && t.plain_blks.size() == t.plain_vertex.size());
	for(size_t i = 0; i < t.long_blks.size() && i < t.long_vertex.size(); ++ i) {
		const int64_t v = t.long_vertex[i];
		CHECK(v >= 0 && v < n);
		if(v < 0 || v >= n) continue;
		Check_Record(t.long_blks[i], true, v);
		CHECK(routes[v] == '?');
		routes[v] = 'L';
		CHECK(c.dims[v] == t.n_long_dim && long_kernel_exists(rd, int(c.dims[v])) && n_v_edges[v] >= LONG_LIST);
		reached.insert("long");
	}
	if(t.long_blks.empty())
		CHECK(t.n_long_dim == 0);
	int n_small_max = 0;
	for(size_t i = 0; i < t.small_blks.size() && i < t.small_vertex.size(); ++ i) {
		const int64_t v = t.small_vertex[i];
		CHECK(v >= 0 && v < n);
		if(v < 0 || v >= n) continue;
		Check_Record(t.small_blks[i], true, v);
		CHECK(routes[v] == '?');
		routes[v] = 'S';
		const int d = int(c.dims[v]);
		CHECK(b_can_pack && 2 * (d * d + d) <= 64);
		n_small_max = std::max(n_small_max, d * d + d);
		reached.insert("small_packed");
	}
	CHECK(t.n_small_elems == n_small_max);
	for(size_t i = 0; i < t.plain_blks.size() && i < t.plain_vertex.size(); ++ i) {
		const int64_t v = t.plain_vertex[i];
		CHECK(v >= 0 && v < n);
		if(v < 0 || v >= n) continue;
		Check_Record(t.plain_blks[i], true, v);
		CHECK(routes[v] == '?');
		routes[v] = 'P';
		const int d = int(c.dims[v]);
		CHECK(!(b_can_pack && 2 * (d * d + d) <= 64));
		CHECK(rd * d <= 56); // assemble_diag_kernel: the lanes of M end where those of the right-hand side begin
		reached.insert("plain_diag");
	}
	for(int64_t v = 0; v < n; ++ v) {
		// the first dimension that qualifies takes the edge-parallel kernel
		if(routes[v] != 'G' && routes[v] != 'L' && n_v_edges[v] >= LONG_LIST && long_kernel_exists(rd, int(c.dims[v]))) {
			CHECK(t.n_long_dim != 0 && t.n_long_dim != c.dims[v]);
			reached.insert("long_dim_taken");
		}
	}
	int n_off_max = 1;
	for(size_t i = 0; i < t.offdiag.size(); ++ i) {
		const int64_t k = Check_Record(t.offdiag[i], false, -1);
		if(k >= 0)
			CHECK(routes[col_of[k]] != 'G');
		n_off_max = std::max(n_off_max, int(t.offdiag[i].rows) * int(t.offdiag[i].cols));
	}
	CHECK(t.n_off_elems == n_off_max);
	const bool b_pack_off = b_can_pack && 2 * t.n_off_elems <= 64; // (assembly_enqueue)
	if(!t.offdiag.empty())
		reached.insert(b_pack_off? "offdiag_packed" : "offdiag_plain");
	// coverage
	for(int64_t k = 0; k < n_blocks; ++ k)
		CHECK(n_block_writes[k] == 1);
	for(int64_t v = 0; v < n; ++ v)
		CHECK(n_eta_writes[v] == 1 && routes[v] != '?');
	printf("%s: info rd=%d d0=%d d1=%d n_groups=%lld n_grp_cap_edges=%d n_grp_pkg_stride=%d n_long=%lld n_long_dim=%d n_small=%lld "
		"n_small_elems=%d n_plain_diag=%lld n_offdiag=%lld n_off_elems=%d b_offdiag_packed=%d routes %s reached", c.name.c_str(), rd, d0, d1,
		(long long)t.n_groups, t.n_grp_cap_edges, t.n_grp_pkg_stride, (long long)t.long_blks.size(), t.n_long_dim,
		(long long)t.small_blks.size(), t.n_small_elems, (long long)t.plain_blks.size(), (long long)t.offdiag.size(), t.n_off_elems,
		int(b_pack_off), routes.c_str());
	for(const std::string &s : reached)
		printf(" %s", s.c_str());
	printf("%s\n", (n_failures == n_fail_before)? " ok" : " FAILED");
}

static int Run_File(const char *p_s_file)
{
	std::ifstream f(p_s_file);
	if(!f) {
		fprintf(stderr, "cannot read %s\n", p_s_file);
		return 2;
	}
	std::string s_word;
	while(f >> s_word) {
		TCase c;
		int64_t n_extra = 0;
		if(s_word != "case" || !(f >> c.name >> c.n >> c.n_edges >> n_extra >> c.rd >> c.n_groups_option) || c.n < 1 || c.n_edges < 1 || n_extra < 0) {
			fprintf(stderr, "bad cases file\n");
			return 2;
		}
		c.dims.resize(c.n); c.v0.resize(c.n_edges); c.v1.resize(c.n_edges);
		std::vector<int64_t> extra(2 * n_extra);
		for(int64_t &x : c.dims) f >> x;
		for(int64_t &x : c.v0) f >> x;
		for(int64_t &x : c.v1) f >> x;
		for(int64_t &x : extra) f >> x;
		if(!f) {
			fprintf(stderr, "bad cases file\n");
			return 2;
		}
		Build_Structure(c, extra);
		try {
			Run_Case(c);
		} catch(std::exception &r_exc) {
			printf("%s: threw %s FAILED\n", c.name.c_str(), r_exc.what());
			++ n_failures;
		}
	}
	return n_failures != 0;
}

// what the builder refuses, and as which exception (capi's guarded() makes SLAMPP_HIP_ERR_INVALID of them)
static int Run_Refusals()
{
	struct TRefusal { const char *p_s_name; int n_kind; }; // 0: invalid_argument, 1: domain_error
	auto Expect = [&](const char *p_s_name, int n_kind, TCase &c, bool b_null = false) {
		TAsmTables t;
		int n_got = -1;
		try {
			assembly_build_tables(t, c.n, c.cs.data(), c.ptr.data(), c.brow.data(), c.n_edges, b_null? 0 : c.v0.data(), c.v1.data(), c.rd, 1 << 20);
		} catch(std::invalid_argument&) {
			n_got = 0;
		} catch(std::domain_error&) {
			n_got = 1;
		}
		CHECK(n_got == n_kind);
		printf("refusal %s: %s%s\n", p_s_name, (n_got == 0)? "invalid_argument" : ((n_got == 1)? "domain_error" : "accepted"), (n_got == n_kind)? " ok" : " FAILED");
	};
	auto Chain = [](int n, int d) {
		TCase c;
		c.n = n; c.n_edges = n - 1; c.rd = 3; c.n_groups_option = -1;
		c.dims.assign(n, d);
		for(int i = 0; i + 1 < n; ++ i) { c.v0.push_back(i); c.v1.push_back(i + 1); }
		Build_Structure(c, std::vector<int64_t>());
		return c;
	};
	{ TCase c = Chain(6, 3); c.v1[2] = 6; Expect("vertex-outside", 0, c); }
	{ TCase c = Chain(6, 3); c.v0[2] = -1; Expect("vertex-negative", 0, c); }
	{ TCase c = Chain(6, 3); c.v1[2] = c.v0[2]; Expect("self-edge", 0, c); }
	{ TCase c = Chain(6, 3); c.v1[0] = 5; Expect("missing-block", 0, c); }
	{ TCase c = Chain(6, 3); // the diagonal block of vertex 0 taken out (an edge-less column would pass the other checks)
		c.brow.erase(c.brow.begin()); for(size_t i = 1; i < c.ptr.size(); ++ i) -- c.ptr[i];
		c.v0.erase(c.v0.begin()); c.v1.erase(c.v1.begin()); -- c.n_edges;
		Expect("missing-diagonal", 0, c); }
	{ TCase c = Chain(6, 8); Expect("dimension-8", 1, c); }
	{ TCase c = Chain(6, 3); c.dims.push_back(8); ++ c.n; Build_Structure(c, std::vector<int64_t>()); Expect("isolated-dimension-8", 1, c); }
	{ TCase c = Chain(6, 3); c.rd = 0; Expect("rd-0", 0, c); }
	{ TCase c = Chain(6, 3); c.rd = 9; Expect("rd-9", 0, c); }
	{ TCase c = Chain(6, 3); c.dims[3] = 4; Build_Structure(c, std::vector<int64_t>()); Expect("unequal-dimensions", 1, c); }
	{ TCase c = Chain(6, 3); c.n_edges = 0; Expect("no-edges", 0, c); }
	{ TCase c = Chain(6, 3); Expect("null-vertices", 0, c, true); }
	return n_failures != 0;
}

static int Run_Sweep()
{
	// assemble_group_kernel<RD, *>: RD = rd for 2, 3, 6, 7, else 0; SZ = 16 for RD 2 and 6, else 4; reached where 4 n_ew >= 8
	std::map<int, std::vector<std::string> > shapes;
	for(int rd = 1; rd <= 8; ++ rd) {
		for(int d0 = 1; d0 <= 7; ++ d0) {
			for(int d1 = 1; d1 <= 7; ++ d1) {
				const TAsmGroupShape t = asm_group_shape(rd, d0, d1);
				CHECK(t.n_ew >= 0 && t.n_ew <= 32 && t.n_instr <= GRP_MAX_INSTR);
				const int n_units = rd * (d0 + d1 + rd + 1) * 8 / ((rd == 2 || rd == 6)? 16 : 4);
				CHECK(t.n_ew * n_units <= 64 * GRP_MAX_INSTR); // what a wave's copy instructions move
				if(4 * t.n_ew >= 8) {
					char p_s[64];
					snprintf(p_s, sizeof(p_s), "(%d,%d,%d):%d", rd, d0, d1, 4 * t.n_ew);
					shapes[(rd == 2 || rd == 3 || rd == 6 || rd == 7)? rd : 0].push_back(p_s);
				}
			}
		}
	}
	const int p_rd[] = {2, 3, 6, 7, 0};
	for(int RD : p_rd) {
		printf("sweep RD=%d SZ=%d shapes=%d", RD, (RD == 2 || RD == 6)? 16 : 4, int(shapes[RD].size()));
		for(size_t i = 0; i < shapes[RD].size() && i < 4; ++ i)
			printf(" %s", shapes[RD][i].c_str());
		printf("%s\n", shapes[RD].empty()? " unreachable" : "");
	}
	for(int rd = 1; rd <= 8; ++ rd) {
		int n_reach = 0, n_cap_max = 0;
		for(int d0 = 1; d0 <= 7; ++ d0)
			for(int d1 = 1; d1 <= 7; ++ d1) {
				const int n_cap = 4 * asm_group_shape(rd, d0, d1).n_ew;
				n_reach += n_cap >= 8;
				n_cap_max = std::max(n_cap_max, n_cap);
			}
		printf("sweep rd=%d grouped_shapes=%d of 49 largest_cap=%d\n", rd, n_reach, n_cap_max);
	}
	return n_failures != 0;
}

int main(int n_arg_num, const char **p_arg_list)
{
	if(n_arg_num == 2 && !strcmp(p_arg_list[1], "refusals"))
		return Run_Refusals();
	if(n_arg_num == 2 && !strcmp(p_arg_list[1], "sweep"))
		return Run_Sweep();
	if(n_arg_num == 2)
		return Run_File(p_arg_list[1]);
	fprintf(stderr, "use: %s <cases file> | refusals | sweep\n", p_arg_list[0]);
	return 2;
}
