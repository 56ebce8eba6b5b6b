// vba_host_posegraph.h -- host half of vba_posegraph_optimize (plain C++17, no HIP): included by vislam_ba.hip (vba_host_small.h)
// and by the sanitizer harness tests/host_posegraph_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_posegraph.py).
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
#include "vba_host_arena.h"
#include "vba_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
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

// One call: the layout and descriptor of every graph and the arena [upload | back | work].  The staging block [desc | estimates |
// measurements | index lists | points] goes up in one copy, [out | estimates | points] come back in one.  One object per call:
// prepare, then describe, pack (any g on any thread), bind, and unpack once the back section is in hout
struct PoseGraphCall {
    bool debug = false;   // set before prepare: graph 0 stops after the solve of its first trial and nothing is written back (hooks flavour)
    int n = 0;
    std::vector<PoseGraphLayout> lay;
    std::vector<PgDesc> desc;
    size_t npt = 0;   // map points of the call
    ArenaLayout L;
    size_t o_desc, o_Sin, o_meas, o_ei, o_ej, o_free, o_vert, o_first, o_last, o_roff, o_incb, o_inc, o_plo, o_phi, o_pb, o_pe, o_pt, o_ref;   // upload
    size_t o_out, o_S, o_pto;                                                                                                                // back
    size_t o_Sbk, o_err, o_J, o_H, o_F, o_Ld, o_b, o_w, o_y, o_x;                                                                            // work

    // 0: every graph is usable and the arena is laid out; otherwise err says which graph is not and why
    int prepare(int n_graphs, const vba_posegraph_problem* const* in, const vba_posegraph_result* const* res, std::string& err) {
        n = n_graphs;
        lay.resize(n);
        desc.resize(n);
        size_t nv = 0, ne = 0, nf = 0, nenv = 0, ninc = 0, npair = 0, npe = 0;
        for (int g = 0; g < n; g++) {
            const std::string who = "graph " + std::to_string(g) + ": ";
            if (!in[g] || !res[g]) { err = who + "NULL problem or result"; return 1; }
            if (build_posegraph(in[g], lay[g], err, (long long)nenv)) { err = who + err; return 1; }
            const vba_posegraph_problem* P = in[g];
            const PoseGraphLayout& G = lay[g];
            PgDesc& d = desc[g];
            std::memset(&d, 0, sizeof d);
            d.nv = P->n_vertices; d.ne = P->n_edges; d.nf = G.n_free; d.npair = (int)G.pair_lo.size();
            d.fix_scale = P->fix_scale ? 1 : 0; d.its = P->its; d.n_pt = P->n_pt; d.debug = (debug && g == 0) ? 1 : 0;
            d.lambda_init = P->lambda_init;
            d.v0 = (long long)nv; d.e0 = (long long)ne; d.f0 = (long long)nf; d.r0 = (long long)nf + g; d.env0 = (long long)nenv;
            d.inc0 = (long long)ninc; d.pair0 = (long long)npair; d.pb0 = (long long)npair + g; d.pe0 = (long long)npe; d.pt0 = (long long)npt;
            nv += (size_t)d.nv; ne += (size_t)d.ne; nf += (size_t)d.nf; nenv += (size_t)G.env_blocks; ninc += G.inc.size();
            npair += G.pair_lo.size(); npe += G.pair_edge.size(); npt += (size_t)d.n_pt;
        }
        auto take = [this](size_t bytes) { return L.take(bytes + 8); };
        const size_t G = (size_t)n;
        o_desc = take(sizeof(PgDesc) * G); o_Sin = take(64 * nv); o_meas = take(64 * ne); o_ei = take(4 * ne); o_ej = take(4 * ne);
        o_free = take(4 * nv); o_vert = take(4 * nf); o_first = take(4 * nf); o_last = take(4 * nf); o_roff = take(4 * (nf + G));
        o_incb = take(4 * (nf + G)); o_inc = take(4 * ninc); o_plo = take(4 * npair); o_phi = take(4 * npair);
        o_pb = take(4 * (npair + G)); o_pe = take(4 * npe); o_pt = take(24 * npt); o_ref = take(4 * npt);
        L.end_upload();
        o_out = take(sizeof(PgOut) * G); o_S = take(64 * nv); o_pto = take(24 * npt);
        L.end_back();
        o_Sbk = take(64 * nv); o_err = take(56 * ne); o_J = take(784 * ne); o_H = take(392 * nenv); o_F = take(392 * nenv);
        o_Ld = take(392 * nf); o_b = take(56 * nf); o_w = take(56 * nf); o_y = take(56 * nf); o_x = take(56 * nf);
        return 0;
    }
    const ArenaLayout& layout() const { return L; }
    size_t download_bytes() const { return L.back_bytes(); }
    size_t grid() const { return (size_t)n; }   // k_posegraph_opt: one workgroup per graph

    // the descriptors were complete with prepare: they go in as one block
    void describe(const vba_posegraph_problem* const*, void* hin) const { std::memcpy(at<char>(hin, o_desc), desc.data(), sizeof(PgDesc) * (size_t)n); }
    // graph g into the staging block: its slices of the concatenated arrays
    const char* pack(int g, const vba_posegraph_problem* P, void* hin) const {
        const PoseGraphLayout& G = lay[g];
        const PgDesc& d = desc[g];
        auto put = [hin](size_t o, size_t off, const void* src, size_t bytes) { if (bytes) std::memcpy(at<char>(hin, o + off), src, bytes); };
        put(o_Sin, 64 * (size_t)d.v0, P->S, 64 * (size_t)d.nv);
        put(o_meas, 64 * (size_t)d.e0, P->edge_S, 64 * (size_t)d.ne);
        put(o_ei, 4 * (size_t)d.e0, P->edge_i, 4 * (size_t)d.ne);
        put(o_ej, 4 * (size_t)d.e0, P->edge_j, 4 * (size_t)d.ne);
        put(o_free, 4 * (size_t)d.v0, G.free_of.data(), 4 * (size_t)d.nv);
        put(o_vert, 4 * (size_t)d.f0, G.vert_of.data(), 4 * (size_t)d.nf);
        put(o_first, 4 * (size_t)d.f0, G.first.data(), 4 * (size_t)d.nf);
        put(o_last, 4 * (size_t)d.f0, G.last_row.data(), 4 * (size_t)d.nf);
        put(o_roff, 4 * (size_t)d.r0, G.row_off.data(), 4 * ((size_t)d.nf + 1));
        put(o_incb, 4 * (size_t)d.r0, G.inc_begin.data(), 4 * ((size_t)d.nf + 1));
        put(o_inc, 4 * (size_t)d.inc0, G.inc.data(), 4 * G.inc.size());
        put(o_plo, 4 * (size_t)d.pair0, G.pair_lo.data(), 4 * G.pair_lo.size());
        put(o_phi, 4 * (size_t)d.pair0, G.pair_hi.data(), 4 * G.pair_hi.size());
        put(o_pb, 4 * (size_t)d.pb0, G.pair_begin.data(), 4 * G.pair_begin.size());
        put(o_pe, 4 * (size_t)d.pe0, G.pair_edge.data(), 4 * G.pair_edge.size());
        put(o_pt, 24 * (size_t)d.pt0, P->pt, 24 * (size_t)d.n_pt);
        int* ref = at<int>(hin, o_ref) + d.pt0;
        for (int p = 0; p < d.n_pt; p++) ref[p] = (int)d.v0 + P->pt_ref[p];   // index into the concatenated vertices
        return nullptr;
    }
    PgBatch bind(void* base) const {
        PgBatch B;
        auto d = [base](size_t o) { return at<double>(base, o); };
        auto i = [base](size_t o) { return at<int>(base, o); };
        B.desc = at<PgDesc>(base, o_desc);
        B.out = at<PgOut>(base, o_out);
        B.Sin = d(o_Sin); B.meas = d(o_meas); B.ei = i(o_ei); B.ej = i(o_ej); B.free_of = i(o_free);
        B.vert_of = i(o_vert); B.first = i(o_first); B.last_row = i(o_last); B.row_off = i(o_roff); B.inc_begin = i(o_incb);
        B.inc = i(o_inc); B.pair_lo = i(o_plo); B.pair_hi = i(o_phi); B.pair_begin = i(o_pb); B.pair_edge = i(o_pe);
        B.pt_in = d(o_pt); B.pt_ref = i(o_ref);
        B.S = d(o_S); B.Sbk = d(o_Sbk); B.err = d(o_err); B.J = d(o_J); B.H = d(o_H); B.F = d(o_F); B.Ld = d(o_Ld);
        B.b = d(o_b); B.w = d(o_w); B.y = d(o_y); B.x = d(o_x); B.pt_out = d(o_pto);
        B.n_pt_total = (long long)npt;
        return B;
    }
    void unpack(int g, vba_posegraph_problem* P, vba_posegraph_result* R, void*, void* hout) const {
        if (debug) return;   // the caller's arrays are left untouched
        const PgDesc& d = desc[g];
        const PgOut& r = at<PgOut>(hout, L.in_back(o_out))[g];
        R->status = r.status; R->its_done = r.its_done; R->lm_trials = r.lm_trials; R->stop = r.stop;
        R->chi2_initial = r.chi2_initial; R->chi2_final = r.chi2_final; R->lambda_final = r.lambda_final;
        if (d.nv) std::memcpy(P->S, at<double>(hout, L.in_back(o_S)) + 8 * (size_t)d.v0, 64 * (size_t)d.nv);   // fixed vertices: the input, bit for bit
        if (d.n_pt) std::memcpy(P->pt, at<double>(hout, L.in_back(o_pto)) + 3 * (size_t)d.pt0, 24 * (size_t)d.n_pt);
    }
};

// the two steps of a call under their earlier names
inline int describe_posegraph(int n_graphs, const vba_posegraph_problem* const* in, const vba_posegraph_result* const* out, bool debug,
                              PoseGraphCall& C, std::string& err) {
    C = PoseGraphCall();
    C.debug = debug;
    return C.prepare(n_graphs, in, out, err);
}
inline void pack_posegraph(const PoseGraphCall& C, int g, const vba_posegraph_problem* P, char* hin) { C.pack(g, P, hin); }

// the envelope blocks of one graph (env, [env_blocks][49]) expanded to the dense symmetric H, [7 n_free]^2 row-major
inline void expand_envelope(const PoseGraphLayout& L, const double* env, double* H) {
    const size_t n = 7 * (size_t)L.n_free;
    std::fill(H, H + n * n, 0.0);
    for (int r = 0; r < L.n_free; r++)
        for (int c = L.first[r]; c <= r; c++) {
            const double* blk = env + 49 * (size_t)(L.row_off[r] + c - L.first[r]);
            for (int a = 0; a < 7; a++)
                for (int k = 0; k < 7; k++) {
                    H[(7 * (size_t)r + a) * n + 7 * (size_t)c + k] = blk[7 * a + k];
                    if (c < r) H[(7 * (size_t)c + k) * n + 7 * (size_t)r + a] = blk[7 * a + k];
                }
        }
}

}  // namespace vba_host
