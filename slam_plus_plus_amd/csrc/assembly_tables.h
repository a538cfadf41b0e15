// assembly_tables.h -- host tables of the Lambda / eta assembly (assembly.hip): which kernel writes which block of Lambda and
// which vertex's eta, and the edge lists they sum, from the structure and the edge set alone.  Host code only: no HIP call,
// nothing of the handle (solver.h); assembly.hip runs the builder and uploads what it made,
// tests/assembly_tables_driver.cpp runs it on the CPU under sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace slampp {

struct TAsmBlk { // 32 B: one block of Lambda and the edges that contribute to it
	int64_t dst;       // offset in the packed Lambda values
	int64_t e0;        // first entry of its edge list
	int64_t eta_off;   // diagonal blocks: scalar offset of the vertex in eta
	int32_t ne;        // number of entries
	int16_t rows, cols;
};

// (residual dimension, vertex dimension) pairs the edge-parallel kernel is instantiated for
inline bool long_kernel_exists(int rd, int d)
{
	return (rd == 2 && (d == 6 || d == 7 || d == 3)) || (rd == 3 && d == 3) || (rd == 6 && d == 6) || (rd == 7 && d == 7);
}

enum { GRP_LDS_BYTES = 160 * 1024 / 6 - 576 - 1536, GRP_PACKAGE_WORDS = 1024, GRP_PKG_PER_THREAD = 4, GRP_MAX_INSTR = 4 }; // LDS of a workgroup (six to a CU); its package; copy instructions per wave // LDS of a group: its edges' records; its package

enum { LONG_LIST = 96 }; // edges of a vertex from which the edge-parallel kernel takes it

// the group kernel's shape for an edge set: bytes of an edge in LDS (J0 | J1 | Sigma^-1 | error as they lie in memory,
// M = Sigma^-1 [J0 J1 e], the weight), edges per wave, copy instructions per wave
struct TAsmGroupShape {
	int n_edge_bytes, n_ew, n_instr;
};

inline TAsmGroupShape asm_group_shape(int rd, int d0, int d1)
{
	const int n_sz = (rd % 2 == 0 && (rd == 2 || rd == 6))? 16 : 4; // (the instantiations with 16-byte copies: assemble_group_kernel's SZ)
	const int n_raw = rd * (d0 + d1 + rd + 1), n_mw = (rd * (d0 + d1 + 1) + 1) & ~1, n_units = n_raw * 8 / n_sz;
	TAsmGroupShape t;
	t.n_edge_bytes = (n_raw + n_mw + 1) * 8;
	t.n_ew = std::min(std::min(int(GRP_LDS_BYTES) / t.n_edge_bytes / 4, 64 * int(GRP_MAX_INSTR) / n_units), 32);
	t.n_instr = (t.n_ew * n_units + 63) / 64;
	return t;
}

// what assembly_setup uploads
struct TAsmTables {
	int d0, d1, rd;
	std::vector<TAsmBlk> offdiag;      // off-diagonal blocks the groups did not take (a single entry rides in e0)
	std::vector<TAsmBlk> long_blks, small_blks, plain_blks; // diagonal blocks of the edge-parallel, the packed and the one-wave kernel
	std::vector<int32_t> long_vertex, small_vertex, plain_vertex; // their vertices
	int n_long_dim;                    // common dimension of the long vertices (0: none qualify)
	int n_small_elems;                 // lanes per vertex in the packed kernel: d^2 + d of the largest of them
	int n_off_elems;                   // largest off-diagonal block, in elements
	std::vector<int32_t> entries;      // edge index * 2 + (off-diagonal: flipped; diagonal: side)
	std::vector<int64_t> edge_state;   // three planes of n_edges: scalar offset of vertex 0, of vertex 1, block column of vertex 0
	int64_t n_groups;
	std::vector<int32_t> grp_words;    // per group, n_grp_pkg_stride words: n_edges, n_blocks, n_entries, n_items | edges (n_grp_cap_edges, padded) | blocks (6 words each) | entries (slot * 2 + flag) | items (two to a word)
	int n_grp_pkg_stride, n_grp_cap_edges;
};

// Lambda of n block columns (cumsum, bcol_ptr, brow: the upper triangle, rows sorted in a column), one homogeneous edge
// set, and the value of option "assembly_groups".  Throws std::invalid_argument / std::domain_error.
void assembly_build_tables(TAsmTables &r_tables, int64_t n, const int64_t *cs, const int64_t *ptr, const int32_t *brow,
	int64_t n_edges, const int64_t *v0, const int64_t *v1, int rd, int n_assembly_groups);

} // namespace slampp
