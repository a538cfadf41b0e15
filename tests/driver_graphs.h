// Test infrastructure: the block graphs of the stand-alone CPU drivers (tests/pair_plan_driver.cpp,
// tests/sparse_records_driver.cpp) and their plans.  Edges are pairs of vertices in any order; the structure handed to
// build_plan() is the upper triangle with the diagonal, rows ascending.
#pragma once
#include "plan.h"
#include <algorithm>
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

typedef std::vector<std::pair<int, int> > CEdgeList;

// the plan of a graph whose vertex i has dimension dims[i % dims.size()]; false (and a line on stdout) if it cannot be built
inline bool plan_of_graph(const char *name, int n, const CEdgeList &edges, const std::vector<int> &dims,
	const slampp::PlanOptions &opt, slampp::Plan &P)
{
	std::vector<std::set<int> > bcols(n);
	for(int i = 0; i < n; ++ i)
		bcols[i].insert(i);
	for(size_t e = 0; e < edges.size(); ++ e) {
		const int a = std::min(edges[e].first, edges[e].second), b = std::max(edges[e].first, edges[e].second);
		if(a != b)
			bcols[b].insert(a);
	}
	std::vector<int64_t> cumsum(n + 1, 0), ptr(n + 1, 0);
	std::vector<int32_t> brow;
	for(int i = 0; i < n; ++ i)
		cumsum[i + 1] = cumsum[i] + dims[size_t(i) % dims.size()];
	for(int c = 0; c < n; ++ c) {
		for(std::set<int>::const_iterator p = bcols[c].begin(); p != bcols[c].end(); ++ p)
			brow.push_back(*p);
		ptr[c + 1] = int64_t(brow.size());
	}
	const std::string err = slampp::build_plan(n, cumsum.data(), ptr.data(), brow.data(), opt, P);
	if(!err.empty()) {
		printf("%s: build_plan: %s\n", name, err.c_str());
		return false;
	}
	return true;
}

// a chain of n vertices with a loop closure every 50 (one draw of the generator each)
inline CEdgeList chain_with_closures(int n, std::mt19937 &rng)
{
	CEdgeList e;
	for(int i = 1; i < n; ++ i)
		e.push_back(std::make_pair(i - 1, i));
	for(int i = 60; i < n; i += 50)
		e.push_back(std::make_pair(i, i - 26 - int(rng() % 30)));
	return e;
}

// a w x w grid, vertex y * w + x
inline CEdgeList grid_graph(int w)
{
	CEdgeList e;
	for(int y = 0; y < w; ++ y) {
		for(int x = 0; x < w; ++ x) {
			if(x)
				e.push_back(std::make_pair(y * w + x - 1, y * w + x));
			if(y)
				e.push_back(std::make_pair((y - 1) * w + x, y * w + x));
		}
	}
	return e;
}

// several pieces and isolated vertices: 2500 random edges among the first 800 of 1500 vertices, a chain over 900 .. 1299
inline CEdgeList pieces_graph(std::mt19937 &rng)
{
	CEdgeList e;
	for(int i = 0; i < 2500; ++ i)
		e.push_back(std::make_pair(int(rng() % 800), int(rng() % 800)));
	for(int i = 901; i < 1300; ++ i)
		e.push_back(std::make_pair(i - 1, i));
	return e;
}
