// assembly_tables.cpp -- the host builder of the Lambda / eta assembly's tables (assembly_tables.h): no device call.
#include "assembly_tables.h"

#include <stdexcept>

namespace slampp {

void assembly_build_tables(TAsmTables &r_tables, int64_t n, const int64_t *cs, const int64_t *ptr, const int32_t *brow,
	int64_t n_edges, const int64_t *v0, const int64_t *v1, int rd, int n_assembly_groups)
{
	if(n_edges <= 0 || !v0 || !v1 || rd <= 0 || rd > 8)
		throw std::invalid_argument("assembly_setup: bad edge set");
	for(int64_t e = 0; e < n_edges; ++ e) {
		if(v0[e] < 0 || v0[e] >= n || v1[e] < 0 || v1[e] >= n || v0[e] == v1[e])
			throw std::invalid_argument("assembly_setup: edge refers to a vertex outside Lambda, or to one vertex twice");
	}
	const int d0 = int(cs[v0[0] + 1] - cs[v0[0]]), d1 = int(cs[v1[0] + 1] - cs[v1[0]]);
	if(d0 > 7 || d1 > 7)
		throw std::domain_error("assembly: vertex dimensions above 7 are not supported");
	for(int64_t e = 0; e < n_edges; ++ e) {
		if(cs[v0[e] + 1] - cs[v0[e]] != d0 || cs[v1[e] + 1] - cs[v1[e]] != d1)
			throw std::domain_error("assembly: all edges of a set must join vertices of the same two dimensions");
	}
	// value offset of every block of Lambda
	std::vector<int64_t> voff(ptr[n] + 1, 0);
	for(int64_t c = 0; c < n; ++ c)
		for(int64_t k = ptr[c]; k < ptr[c + 1]; ++ k)
			voff[k + 1] = voff[k] + (cs[brow[k] + 1] - cs[brow[k]]) * (cs[c + 1] - cs[c]);
	// edge lists per block: count, then fill (stable: edges stay in their given order inside a list)
	std::vector<int64_t> blk_of_edge(n_edges);
	std::vector<int32_t> cnt_off(ptr[n], 0), cnt_diag(n, 0);
	for(int64_t e = 0; e < n_edges; ++ e) {
		const int64_t r = std::min(v0[e], v1[e]), c = std::max(v0[e], v1[e]);
		const int32_t *b = std::lower_bound(brow + ptr[c], brow + ptr[c + 1], int32_t(r));
		if(b == brow + ptr[c + 1] || *b != r)
			throw std::invalid_argument("assembly_setup: Lambda has no block for an edge");
		blk_of_edge[e] = b - brow;
		++ cnt_off[b - brow];
		++ cnt_diag[v0[e]];
		++ cnt_diag[v1[e]];
	}
	std::vector<TAsmBlk> offdiag, diag(n);
	std::vector<int64_t> off_slot(ptr[n], -1);
	int64_t n_entries = 0;
	for(int64_t c = 0; c < n; ++ c) {
		for(int64_t k = ptr[c]; k < ptr[c + 1]; ++ k) {
			if(brow[k] == c)
				continue;
			TAsmBlk b;
			b.dst = voff[k]; b.e0 = n_entries; b.ne = cnt_off[k]; b.eta_off = 0;
			b.rows = int16_t(cs[brow[k] + 1] - cs[brow[k]]); b.cols = int16_t(cs[c + 1] - cs[c]);
			n_entries += cnt_off[k];
			off_slot[k] = int64_t(offdiag.size());
			offdiag.push_back(b); // blocks without an edge are written as zeros
		}
	}
	for(int64_t v = 0; v < n; ++ v) {
		if(ptr[v + 1] == ptr[v] || brow[ptr[v + 1] - 1] != v)
			throw std::invalid_argument("assembly_setup: a diagonal block is missing");
		TAsmBlk &b = diag[v];
		b.dst = voff[ptr[v + 1] - 1]; b.e0 = n_entries; b.ne = cnt_diag[v]; b.eta_off = cs[v];
		b.rows = b.cols = int16_t(cs[v + 1] - cs[v]);
		if(b.rows > 7)
			throw std::domain_error("assembly: vertex dimensions above 7 are not supported");
		n_entries += cnt_diag[v];
	}
	if(n_edges >= (int64_t(1) << 30))
		throw std::domain_error("assembly: too many edges");
	std::vector<int32_t> entries(n_entries);
	{
		std::vector<int64_t> fill_off(offdiag.size()), fill_diag(n);
		for(size_t i = 0; i < offdiag.size(); ++ i) fill_off[i] = offdiag[i].e0;
		for(int64_t v = 0; v < n; ++ v) fill_diag[v] = diag[v].e0;
		for(int64_t e = 0; e < n_edges; ++ e) {
			entries[fill_off[off_slot[blk_of_edge[e]]] ++] = int32_t(e * 2 + (v0[e] > v1[e]));
			entries[fill_diag[v0[e]] ++] = int32_t(e * 2);
			entries[fill_diag[v1[e]] ++] = int32_t(e * 2 + 1);
		}
	}
	// Groups of consecutive vertices (a pose graph's odometry chain makes neighbours of them): the workgroup of a group
	// brings the records of all edges that touch its vertices into LDS once and writes every block of their columns --
	// an edge inside a group is read once instead of three times (off-diagonal block, two diagonal blocks), one that
	// leaves it twice.  A group closes at GRP_VERTICES vertices or when its edges would not fit; vertices with more edges
	// than fit on their own stay with the kernels below.
	std::vector<int64_t> grp_ptr;
	std::vector<int32_t> grp_words;
	std::vector<uint8_t> b_grouped(n, 0);
	int n_grp_pkg_cap = 0, n_grp_cap_edges = 0;
	{
		const int n_grp_vertices = n_assembly_groups; // option "assembly_groups": as many as fit by default, 0 = the one-wave kernels for everything
		const int n_mode = n_grp_vertices > 0;
		const TAsmGroupShape t_shape = asm_group_shape(rd, d0, d1);
		const int n_cap_edges = 4 * t_shape.n_ew; // as many edges as the workgroup copies in one go: n_ew per wave
		n_grp_cap_edges = n_cap_edges;
		if(n_mode > 0 && n_cap_edges >= 8) {
			std::vector<int64_t> stamp(n_edges, -1);
			std::vector<int32_t> slot_of(n_edges, 0);
			std::vector<int32_t> g_edges, g_blocks, g_entries;
			std::vector<uint16_t> g_items;
			std::vector<int64_t> g_vertices;
			auto Close = [&]() {
				if(g_vertices.empty())
					return;
				g_blocks.clear(); g_entries.clear(); g_items.clear();
				for(size_t i = 0; i < g_vertices.size(); ++ i) {
					const int64_t v = g_vertices[i];
					for(int64_t k = ptr[v]; k < ptr[v + 1]; ++ k) {
						const bool b_diag = brow[k] == v;
						const TAsmBlk &b = b_diag? diag[v] : offdiag[off_slot[k]];
						const int32_t n_begin = int32_t(g_entries.size());
						for(int64_t i2 = 0; i2 < b.ne; ++ i2) {
							const int32_t ent = entries[b.e0 + i2];
							g_entries.push_back(slot_of[ent >> 1] * 2 + (ent & 1));
						}
						g_blocks.push_back(int32_t(uint64_t(b.dst) & 0xffffffffu));
						g_blocks.push_back(int32_t(uint64_t(b.dst) >> 32));
						g_blocks.push_back(b_diag? int32_t(b.eta_off) : -1);
						g_blocks.push_back(int32_t(v));
						g_blocks.push_back(n_begin | (int32_t(b.ne) << 16));
						g_blocks.push_back(int32_t(b.rows) | (int32_t(b.cols) << 8));
						for(int q = 0; q < int(b.cols) + (b_diag? 1 : 0); ++ q)
							g_items.push_back(uint16_t((g_blocks.size() / 6 - 1) * 8 + q)); // (block, column; column `cols` of a diagonal block: eta)
					}
					b_grouped[v] = 1;
				}
				// the lanes of a wave walk their blocks' edge lists in step: blocks with lists of the same length next to each other
				std::stable_sort(g_items.begin(), g_items.end(), [&](uint16_t a, uint16_t b) {
					return (uint32_t(g_blocks[6 * (a >> 3) + 4]) >> 16) < (uint32_t(g_blocks[6 * (b >> 3) + 4]) >> 16); });
				grp_ptr.push_back(int64_t(grp_words.size()));
				grp_words.push_back(int32_t(g_edges.size()));
				grp_words.push_back(int32_t(g_blocks.size() / 6));
				grp_words.push_back(int32_t(g_entries.size()));
				grp_words.push_back(int32_t(g_items.size()));
				grp_words.insert(grp_words.end(), g_edges.begin(), g_edges.end());
				grp_words.insert(grp_words.end(), size_t(n_cap_edges) - g_edges.size(), g_edges.empty()? 0 : g_edges[0]); // (valid addresses for the requests)
				grp_words.insert(grp_words.end(), g_blocks.begin(), g_blocks.end());
				grp_words.insert(grp_words.end(), g_entries.begin(), g_entries.end());
				for(size_t i = 0; i < g_items.size(); i += 2)
					grp_words.push_back(int32_t(uint32_t(g_items[i]) | (uint32_t((i + 1 < g_items.size())? g_items[i + 1] : 0) << 16)));
				n_grp_pkg_cap = std::max(n_grp_pkg_cap, int(4 + n_cap_edges + g_blocks.size() + g_entries.size() + (g_items.size() + 1) / 2));
				g_edges.clear(); g_vertices.clear();
			};
			int64_t n_group = 0, n_group_words = 0; // number of the open group; words of its blocks and entries so far
			for(int64_t v = 0; v < n; ++ v) {
				const int64_t n_v_words = (6 + 4) * (ptr[v + 1] - ptr[v]) + 3 * int64_t(cnt_diag[v]) + 1; // blocks and their items, entries
				if(cnt_diag[v] > n_cap_edges || n_v_words + 4 + n_cap_edges > GRP_PACKAGE_WORDS || int(diag[v].rows) * int(diag[v].rows) + int(diag[v].rows) > 64) {
					Close(); // (consecutive vertices only)
					++ n_group; n_group_words = 0;
					continue;
				}
				int n_new = 0;
				for(int64_t i = 0; i < diag[v].ne; ++ i)
					n_new += stamp[entries[diag[v].e0 + i] >> 1] != n_group;
				if(int(g_vertices.size()) == n_grp_vertices || int(g_edges.size()) + n_new > n_cap_edges ||
				   n_group_words + n_v_words + 4 + n_cap_edges > GRP_PACKAGE_WORDS) {
					Close();
					++ n_group; n_group_words = 0;
				}
				for(int64_t i = 0; i < diag[v].ne; ++ i) {
					const int64_t e = entries[diag[v].e0 + i] >> 1;
					if(stamp[e] != n_group) {
						stamp[e] = n_group;
						slot_of[e] = int32_t(g_edges.size());
						g_edges.push_back(int32_t(e));
					}
				}
				g_vertices.push_back(v);
				n_group_words += n_v_words;
			}
			Close();
			grp_ptr.push_back(int64_t(grp_words.size()));
			if(grp_ptr.size() == 1)
				grp_ptr.clear();
			else { // one stride for all packages: a workgroup finds its next one without a lookup
				n_grp_pkg_cap = (n_grp_pkg_cap + 3) & ~3; // (the records behind it start at a multiple of 16 bytes)
				std::vector<int32_t> t_fixed((grp_ptr.size() - 1) * size_t(n_grp_pkg_cap), 0);
				for(size_t i = 0; i + 1 < grp_ptr.size(); ++ i)
					std::copy(grp_words.begin() + grp_ptr[i], grp_words.begin() + grp_ptr[i + 1], t_fixed.begin() + i * size_t(n_grp_pkg_cap));
				grp_words.swap(t_fixed);
			}
			// the kernels below keep what the groups did not take
			std::vector<TAsmBlk> offdiag_rest;
			for(int64_t c = 0; c < n; ++ c) {
				if(b_grouped[c])
					continue;
				for(int64_t k = ptr[c]; k < ptr[c + 1]; ++ k)
					if(brow[k] != c) offdiag_rest.push_back(offdiag[off_slot[k]]);
			}
			offdiag.swap(offdiag_rest);
		}
	}
	// Three kernels share the vertices: long lists go to the edge-parallel kernel (one lane per edge, tree reduction)
	// when it exists for their dimension; low-dimensional vertices with short lists (the landmarks of a BA system:
	// 12 of 64 lanes busy otherwise) are packed several to a wave when the residual is small enough to unroll; the
	// rest stay with one wave per vertex
	std::vector<TAsmBlk> long_blks, small_blks, plain_blks;
	std::vector<int32_t> long_vertex, small_vertex, plain_vertex;
	int n_long_dim = 0, n_small_elems = 0;
	{
		const bool b_can_pack = rd == 2 || rd == 3;
		for(int64_t v = 0; v < n; ++ v) {
			const int d = diag[v].rows;
			if(b_grouped[v])
				continue;
			if(diag[v].ne >= LONG_LIST && long_kernel_exists(rd, d) && (!n_long_dim || d == n_long_dim)) {
				n_long_dim = d;
				long_blks.push_back(diag[v]);
				long_vertex.push_back(int32_t(v));
			} else if(b_can_pack && 2 * (d * d + d) <= 64) {
				n_small_elems = std::max(n_small_elems, d * d + d);
				small_blks.push_back(diag[v]);
				small_vertex.push_back(int32_t(v));
			} else {
				plain_blks.push_back(diag[v]);
				plain_vertex.push_back(int32_t(v));
			}
		}
	}
	int n_off_elems = 1;
	for(size_t i = 0; i < offdiag.size(); ++ i) {
		n_off_elems = std::max(n_off_elems, int(offdiag[i].rows) * int(offdiag[i].cols));
		if(offdiag[i].ne == 1)
			offdiag[i].e0 = entries[offdiag[i].e0]; // a single entry rides in the record: one dependent load less
	}
	std::vector<int64_t> edge_state(size_t(3 * n_edges));
	for(int64_t e = 0; e < n_edges; ++ e) {
		edge_state[e] = cs[v0[e]];
		edge_state[n_edges + e] = cs[v1[e]];
		edge_state[2 * n_edges + e] = v0[e];
	}
	r_tables.d0 = d0; r_tables.d1 = d1; r_tables.rd = rd;
	r_tables.offdiag.swap(offdiag);
	r_tables.long_blks.swap(long_blks); r_tables.small_blks.swap(small_blks); r_tables.plain_blks.swap(plain_blks);
	r_tables.long_vertex.swap(long_vertex); r_tables.small_vertex.swap(small_vertex); r_tables.plain_vertex.swap(plain_vertex);
	r_tables.n_long_dim = n_long_dim; r_tables.n_small_elems = n_small_elems; r_tables.n_off_elems = n_off_elems;
	r_tables.entries.swap(entries);
	r_tables.edge_state.swap(edge_state);
	r_tables.n_groups = grp_ptr.empty()? 0 : int64_t(grp_ptr.size()) - 1;
	r_tables.grp_words.swap(grp_words);
	r_tables.n_grp_pkg_stride = n_grp_pkg_cap; r_tables.n_grp_cap_edges = n_grp_cap_edges;
}

} // namespace slampp
