// vba_host_posegraph.h -- host half of vba_posegraph_optimize (plain C++17, no HIP): included by vislam_ba.hip and by the
// sanitizer harness tests/host_posegraph_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_posegraph.py).
//
// One walk validates a graph of Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:4243-4552: VertexSim3Expmap per keyframe,
// EdgeSim3 per pair) and lays out its linear system:
//   * free vertices are numbered in the caller's order (keyframe ids are temporal: already a good elimination order; there is no
//     reordering);
//   * block row r of H (7x7 blocks, lower triangle) stores the blocks first[r] .. r, first[r] = the smallest free index among r and
//     its neighbours.  The fill of an L D L^T in this order stays inside that envelope, so there is no symbolic factorisation;
//   * every H block and every b segment has ONE owner that sums its edges in edge order: the per-vertex incidence list (diagonal
//     block and b) and the list of distinct free pairs (off-diagonal blocks).
//
// Size bound: the envelopes of all graphs of one call hold at most PG_MAX_ENV_BLOCKS = 2^21 blocks (the device keeps H and its
// factor: 2 x 2^21 x 49 x 8 bytes = 1.6 GB).  A 5 000-vertex graph with a 40-keyframe band and a loop of 8 edges over its whole
// length has about 5 000 x 41 + 8 x 5 000 = 245 000 blocks, an eighth of the bound.
#pragma once
#include "../../include/vislam_ba.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace vba_host {

constexpr long long PG_MAX_ENV_BLOCKS = 1LL << 21;

struct PoseGraphLayout {
    int n_free = 0;
    long long env_blocks = 0;          // row_off[n_free]
    std::vector<int> free_of;          // [n_vertices] free index, -1 for a fixed vertex
    std::vector<int> vert_of;          // [n_free] the caller's index
    std::vector<int> first;            // [n_free] first block column of row r
    std::vector<int> row_off;          // [n_free + 1] block offset of row r; block (r, c) sits at row_off[r] + c - first[r]
    std::vector<int> last_row;         // [n_free] the largest row whose envelope reaches column c (>= c)
    std::vector<int> inc_begin, inc;   // per free vertex its edges in edge order, as 2 * edge + side (0: vertex 0 of the edge, 1: vertex 1)
    // distinct pairs of free vertices joined by an edge, sorted by (hi, lo); their edges in edge order as 2 * edge + s,
    // s = 1 when hi is vertex 0 of that edge
    std::vector<int> pair_lo, pair_hi, pair_begin, pair_edge;
};

namespace pg_detail {
inline const char* check_sim3(const double* S, const char* what_finite, const char* what_q, const char* what_s) {
    for (int k = 0; k < 8; k++)
        if (!std::isfinite(S[k])) return what_finite;
    if (!(S[3] * S[3] + S[4] * S[4] + S[5] * S[5] + S[6] * S[6] > 0.0)) return what_q;
    if (!(S[7] > 0.0)) return what_s;
    return nullptr;
}
}  // namespace pg_detail

// 0: the graph is usable and L describes it; otherwise err says why not.  env_before: envelope blocks of the graphs of the same
// call that came before (the bound holds for the call).
inline int build_posegraph(const vba_posegraph_problem* P, PoseGraphLayout& L, std::string& err, long long env_before = 0) {
    auto fail = [&err](const std::string& m) { err = m; return 1; };
    if (!P) return fail("NULL problem");
    if (P->n_vertices < 0 || P->n_edges < 0 || P->n_pt < 0) return fail("negative count");
    if ((P->n_vertices > 0 && (!P->S || !P->fixed)) || (P->n_edges > 0 && (!P->edge_i || !P->edge_j || !P->edge_S)) ||
        (P->n_pt > 0 && (!P->pt || !P->pt_ref)))
        return fail("NULL array with a non-zero count");
    if (P->its < 1) return fail("its must be at least 1");
    if (!(P->lambda_init > 0.0) || !std::isfinite(P->lambda_init)) return fail("lambda_init must be positive");
    const int nv = P->n_vertices, ne = P->n_edges;
    for (int v = 0; v < nv; v++)
        if (const char* m = pg_detail::check_sim3(P->S + 8 * (size_t)v, "S is not finite", "zero quaternion in S", "scale of S is not positive"))
            return fail(std::string(m) + " (vertex " + std::to_string(v) + ")");
    L = PoseGraphLayout();
    L.free_of.assign(nv, -1);
    for (int v = 0; v < nv; v++)
        if (!P->fixed[v]) {
            L.free_of[v] = L.n_free++;
            L.vert_of.push_back(v);
        }
    if (L.n_free == 0) return fail("no free vertex");
    for (int e = 0; e < ne; e++) {
        const int i = P->edge_i[e], j = P->edge_j[e];
        const std::string at = " (edge " + std::to_string(e) + ")";
        if (i < 0 || i >= nv || j < 0 || j >= nv) return fail("edge index out of range" + at);
        if (i == j) return fail("edge_i == edge_j" + at);
        if (P->fixed[i] && P->fixed[j]) return fail("edge between two fixed vertices" + at);
        if (const char* m = pg_detail::check_sim3(P->edge_S + 8 * (size_t)e, "edge_S is not finite", "zero quaternion in edge_S", "scale of edge_S is not positive"))
            return fail(std::string(m) + at);
    }
    for (int p = 0; p < P->n_pt; p++) {
        if (P->pt_ref[p] < 0 || P->pt_ref[p] >= nv) return fail("pt_ref out of range (point " + std::to_string(p) + ")");
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(P->pt[3 * (size_t)p + k])) return fail("pt is not finite (point " + std::to_string(p) + ")");
    }
    const int nf = L.n_free;
    // envelope
    L.first.resize(nf);
    for (int r = 0; r < nf; r++) L.first[r] = r;
    std::vector<int> cnt(nf + 1, 0);
    size_t n_pair_edges = 0;
    for (int e = 0; e < ne; e++) {
        const int a = L.free_of[P->edge_i[e]], b = L.free_of[P->edge_j[e]];
        if (a >= 0) cnt[a + 1]++;
        if (b >= 0) cnt[b + 1]++;
        if (a >= 0 && b >= 0) {
            const int hi = std::max(a, b), lo = std::min(a, b);
            L.first[hi] = std::min(L.first[hi], lo);
            n_pair_edges++;
        }
    }
    L.row_off.resize(nf + 1);
    long long off = 0;
    for (int r = 0; r < nf; r++) {
        L.row_off[r] = (int)off;
        off += r - L.first[r] + 1;
        if (env_before + off > PG_MAX_ENV_BLOCKS)
            return fail("the envelope of the factor exceeds the bound of " + std::to_string(PG_MAX_ENV_BLOCKS) + " blocks for one call");
    }
    L.row_off[nf] = (int)off;
    L.env_blocks = off;
    L.last_row.resize(nf);
    for (int c = 0; c < nf; c++) L.last_row[c] = c;
    for (int r = 0; r < nf; r++) L.last_row[L.first[r]] = std::max(L.last_row[L.first[r]], r);
    for (int c = 1; c < nf; c++) L.last_row[c] = std::max(L.last_row[c], L.last_row[c - 1]);
    // incidence lists, edge order
    L.inc_begin.assign(nf + 1, 0);
    for (int r = 0; r < nf; r++) L.inc_begin[r + 1] = L.inc_begin[r] + cnt[r + 1];
    L.inc.resize(L.inc_begin[nf]);
    std::vector<int> fill(L.inc_begin.begin(), L.inc_begin.end() - 1);
    for (int e = 0; e < ne; e++) {
        const int a = L.free_of[P->edge_i[e]], b = L.free_of[P->edge_j[e]];
        if (a >= 0) L.inc[fill[a]++] = 2 * e;
        if (b >= 0) L.inc[fill[b]++] = 2 * e + 1;
    }
    // distinct free pairs, their edges in edge order
    struct PE { int hi, lo, e, s; };
    std::vector<PE> pe;
    pe.reserve(n_pair_edges);
    for (int e = 0; e < ne; e++) {
        const int a = L.free_of[P->edge_i[e]], b = L.free_of[P->edge_j[e]];
        if (a >= 0 && b >= 0) pe.push_back(PE{std::max(a, b), std::min(a, b), e, a > b ? 1 : 0});
    }
    std::sort(pe.begin(), pe.end(), [](const PE& x, const PE& y) {
        if (x.hi != y.hi) return x.hi < y.hi;
        if (x.lo != y.lo) return x.lo < y.lo;
        return x.e < y.e;
    });
    for (size_t k = 0; k < pe.size(); k++) {
        if (k == 0 || pe[k].hi != pe[k - 1].hi || pe[k].lo != pe[k - 1].lo) {
            L.pair_hi.push_back(pe[k].hi);
            L.pair_lo.push_back(pe[k].lo);
            L.pair_begin.push_back((int)k);
        }
        L.pair_edge.push_back(2 * pe[k].e + pe[k].s);
    }
    L.pair_begin.push_back((int)pe.size());
    return 0;
}

}  // namespace vba_host
