// Sanitizer harness of the host half of vba_posegraph_optimize (mc_slam_amd/csrc/vba_host_posegraph.h): plain C++, built by
// tests/test_host_posegraph.py with g++ -fsanitize=address,undefined.
//   host_posegraph_check <file>...            -> one line per file: "ok <summary>" or "error <message>"
//   host_posegraph_check --call <file>...     -> the files as the graphs of one call: sizes and the arena offsets in arena order
//   host_posegraph_check --expand <file>      -> the dense expansion of the graph's envelope (expand_envelope)
// File (little-endian, written by the test): i32 n_vertices n_edges fix_scale its n_pt mutate, f64 lambda_init, f64 env_before,
// then S [nv][8] f64, fixed [nv] u8, edge_i [ne] i32, edge_j [ne] i32, edge_S [ne][8] f64, pt [n_pt][3] f64, pt_ref [n_pt] i32.
// mutate: 0 nothing, 1 n_vertices = -1, 2 n_edges = -1, 3 n_pt = -1, 4 S = NULL, 5 edge_S = NULL, 6 pt = NULL, 7 fixed = NULL.
#include "../mc_slam_amd/csrc/vba_host_posegraph.h"

#include "host_check.h"

#include <set>

template <class T>
static bool take(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static const char* invariants(const vba_posegraph_problem& P, const vba_host::PoseGraphLayout& L) {
    const int nf = L.n_free;
    if ((int)L.free_of.size() != P.n_vertices || (int)L.vert_of.size() != nf || (int)L.first.size() != nf || (int)L.row_off.size() != nf + 1 ||
        (int)L.last_row.size() != nf || (int)L.inc_begin.size() != nf + 1)
        return "sizes";
    int k = 0;
    for (int v = 0; v < P.n_vertices; v++) {   // free vertices numbered in the caller's order
        if (P.fixed[v] ? L.free_of[v] != -1 : (L.free_of[v] != k || L.vert_of[k] != v)) return "free numbering";
        if (!P.fixed[v]) k++;
    }
    if (k != nf || L.row_off[0] != 0) return "free count";
    for (int r = 0; r < nf; r++) {
        if (L.first[r] < 0 || L.first[r] > r) return "first[r] <= r";
        if (L.row_off[r + 1] - L.row_off[r] != r - L.first[r] + 1) return "offsets";
        if (L.last_row[r] < r || L.last_row[r] >= nf) return "last_row range";
        if (L.inc_begin[r] > L.inc_begin[r + 1]) return "inc_begin";
    }
    if (L.env_blocks != L.row_off[nf] || L.inc_begin[nf] != (int)L.inc.size()) return "totals";
    for (int c = 0; c < nf; c++)
        for (int r = c; r < nf; r++)
            if ((L.first[r] <= c) != (r <= L.last_row[c]) && L.first[r] <= c) return "last_row misses a row";
    std::vector<int> first_seen(nf);
    for (int r = 0; r < nf; r++) first_seen[r] = r;
    size_t n_inc = 0, n_pe = 0;
    for (int e = 0; e < P.n_edges; e++) {   // every edge inside the envelope of its later row
        const int a = L.free_of[P.edge_i[e]], b = L.free_of[P.edge_j[e]];
        n_inc += (a >= 0) + (b >= 0);
        if (a < 0 || b < 0) continue;
        n_pe++;
        const int hi = std::max(a, b), lo = std::min(a, b);
        if (L.first[hi] > lo) return "edge outside the envelope";
        first_seen[hi] = std::min(first_seen[hi], lo);
    }
    for (int r = 0; r < nf; r++)
        if (first_seen[r] != L.first[r]) return "envelope wider than its edges";
    if (n_inc != L.inc.size() || n_pe != L.pair_edge.size()) return "list totals";
    for (int r = 0; r < nf; r++)   // incidence lists: the vertex' own edges, in edge order
        for (int q = L.inc_begin[r]; q < L.inc_begin[r + 1]; q++) {
            const int e = L.inc[q] >> 1, s = L.inc[q] & 1;
            if (e < 0 || e >= P.n_edges || (s ? P.edge_j[e] : P.edge_i[e]) != L.vert_of[r]) return "incidence entry";
            if (q > L.inc_begin[r] && L.inc[q - 1] >= L.inc[q]) return "incidence order";
        }
    const size_t np = L.pair_lo.size();
    if (L.pair_hi.size() != np || L.pair_begin.size() != np + 1 || L.pair_begin[0] != 0 || L.pair_begin[np] != (int)L.pair_edge.size()) return "pair sizes";
    std::set<std::pair<int, int>> seen;
    for (size_t p = 0; p < np; p++) {
        const int hi = L.pair_hi[p], lo = L.pair_lo[p];
        if (lo < 0 || lo >= hi || hi >= nf || !seen.insert({hi, lo}).second) return "pair not distinct";
        if (L.pair_begin[p] >= L.pair_begin[p + 1]) return "empty pair";
        for (int q = L.pair_begin[p]; q < L.pair_begin[p + 1]; q++) {
            const int e = L.pair_edge[q] >> 1, s = L.pair_edge[q] & 1;
            if (e < 0 || e >= P.n_edges) return "pair edge range";
            const int a = L.free_of[P.edge_i[e]], b = L.free_of[P.edge_j[e]];
            if ((s ? a : b) != hi || (s ? b : a) != lo) return "pair edge";
            if (q > L.pair_begin[p] && (L.pair_edge[q - 1] >> 1) >= e) return "pair edge order";
        }
    }
    return nullptr;
}

// one file: the caller's arrays and the problem that points at them
struct Graph {
    std::vector<double> S, M, pt;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> ei, ej, ref;
    vba_posegraph_problem P;
    double env_before = 0;
    bool load(const char* path) {
        FILE* f = fopen(path, "rb");
        int32_t hd[6];
        double sc[2];
        if (!f || fread(hd, 4, 6, f) != 6 || fread(sc, 8, 2, f) != 2) { if (f) fclose(f); return false; }
        const size_t nv = hd[0], ne = hd[1], np = hd[4];
        const bool ok = take(f, S, 8 * nv) && take(f, fixed, nv) && take(f, ei, ne) && take(f, ej, ne) && take(f, M, 8 * ne) && take(f, pt, 3 * np) && take(f, ref, np);
        fclose(f);
        if (!ok) return false;
        std::memset(&P, 0, sizeof P);
        P.n_vertices = hd[0]; P.n_edges = hd[1]; P.fix_scale = hd[2]; P.its = hd[3]; P.n_pt = hd[4];
        P.lambda_init = sc[0];
        env_before = sc[1];
        P.S = S.data(); P.fixed = fixed.data(); P.edge_i = ei.data(); P.edge_j = ej.data(); P.edge_S = M.data(); P.pt = pt.data(); P.pt_ref = ref.data();
        switch (hd[5]) {
            case 1: P.n_vertices = -1; break;
            case 2: P.n_edges = -1; break;
            case 3: P.n_pt = -1; break;
            case 4: P.S = nullptr; break;
            case 5: P.edge_S = nullptr; break;
            case 6: P.pt = nullptr; break;
            case 7: P.fixed = nullptr; break;
            default: break;
        }
        return true;
    }
};

// --call <file>...: the files as the graphs of ONE call, PoseGraphCall run as the library's driver runs it (run_call,
// tests/host_check.h) -- its sizes, the offset of every region of the arena in arena order, and where the kernel's argument points
static void one_call(int n, char** files) {
    std::vector<Graph> G(n);
    std::vector<vba_posegraph_problem*> pp(n);
    std::vector<vba_posegraph_result> R(n);
    std::vector<vba_posegraph_result*> rr(n);
    for (int g = 0; g < n; g++) {
        if (!G[g].load(files[g])) { printf("error load\n"); return; }
        pp[g] = &G[g].P; rr[g] = &R[g];
    }
    Heap H;
    vba_host::PoseGraphCall C;
    size_t nv = 0;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const PgBatch& B, void* hin) {
        size_t ne = 0, nf = 0, nenv = 0, ninc = 0, npair = 0, npe = 0;
        for (int g = 0; g < n; g++) {
            const vba_host::PoseGraphLayout& L = C.lay[g];
            nv += G[g].P.n_vertices; ne += G[g].P.n_edges; nf += L.n_free; nenv += L.env_blocks; ninc += L.inc.size(); npair += L.pair_lo.size(); npe += L.pair_edge.size();
        }
        printf("call nv %zu ne %zu nf %zu nenv %zu ninc %zu npair %zu npe %zu npt %zu upload %zu back %zu total %zu offsets", nv, ne, nf, nenv, ninc, npair, npe, C.npt,
               C.L.upload_bytes(), C.L.back_bytes(), C.L.total_bytes());
        for (size_t o : {C.o_desc, C.o_Sin, C.o_meas, C.o_ei, C.o_ej, C.o_free, C.o_vert, C.o_first, C.o_last, C.o_roff, C.o_incb, C.o_inc, C.o_plo, C.o_phi, C.o_pb,
                         C.o_pe, C.o_pt, C.o_ref, C.o_out, C.o_S, C.o_pto, C.o_Sbk, C.o_err, C.o_J, C.o_H, C.o_F, C.o_Ld, C.o_b, C.o_w, C.o_y, C.o_x})
            printf(" %zu", o);
        // the last point reference of the last graph, as packed: an index into the concatenated vertices
        printf(" last_ref %d", C.npt ? vba_host::at<int>(hin, C.o_ref)[C.npt - 1] : -1);
        // where every pointer of the kernel's argument points, in arena order
        printf(" bind");
        for (const void* p : {(const void*)B.desc, (const void*)B.Sin, (const void*)B.meas, (const void*)B.ei, (const void*)B.ej, (const void*)B.free_of,
                              (const void*)B.vert_of, (const void*)B.first, (const void*)B.last_row, (const void*)B.row_off, (const void*)B.inc_begin,
                              (const void*)B.inc, (const void*)B.pair_lo, (const void*)B.pair_hi, (const void*)B.pair_begin, (const void*)B.pair_edge,
                              (const void*)B.pt_in, (const void*)B.pt_ref, (const void*)B.out, (const void*)B.S, (const void*)B.pt_out, (const void*)B.Sbk,
                              (const void*)B.err, (const void*)B.J, (const void*)B.H, (const void*)B.F, (const void*)B.Ld, (const void*)B.b, (const void*)B.w,
                              (const void*)B.y, (const void*)B.x})
            printf(" %zu", (size_t)((const char*)p - (const char*)hin));
        printf(" n_pt_total %lld", B.n_pt_total);
    }, [&](void* hout) {
        // what came back: graph g stopped after g iterations, double j of the estimates is j, double j of the points is -j
        PgOut* res = vba_host::at<PgOut>(hout, C.L.in_back(C.o_out));
        double* S = vba_host::at<double>(hout, C.L.in_back(C.o_S));
        double* pt = vba_host::at<double>(hout, C.L.in_back(C.o_pto));
        for (int g = 0; g < n; g++) { std::memset(&res[g], 0, sizeof res[g]); res[g].its_done = g; }
        for (size_t j = 0; j < 8 * nv; j++) S[j] = (double)j;
        for (size_t j = 0; j < 3 * C.npt; j++) pt[j] = -(double)j;
    });
    if (!ran) return;
    double s_S = 0, s_pt = 0;
    long long s_its = 0;
    for (int g = 0; g < n; g++) {
        s_its += R[g].its_done;
        for (double v : G[g].S) s_S += v;
        for (double v : G[g].pt) s_pt += v;
    }
    printf(" got_its %lld got_S %.0f got_pt %.0f\n", s_its, s_S, s_pt);
}

// --expand <file>: envelope block q holds 100 q + 7 a + k + 1 at (a, k) below the diagonal; the dense expansion, row by row
static void expand(const char* file) {
    Graph G;
    vba_host::PoseGraphLayout L;
    std::string err;
    if (!G.load(file) || vba_host::build_posegraph(&G.P, L, err)) { printf("error %s\n", err.c_str()); return; }
    std::vector<double> env(49 * (size_t)L.env_blocks), H(49 * (size_t)L.n_free * L.n_free, -1.0);
    for (size_t q = 0; q < env.size(); q++) env[q] = 100.0 * (double)(q / 49) + (double)(q % 49) + 1.0;
    for (int r = 0; r < L.n_free; r++) {   // a diagonal block is symmetric itself: 100 q + 7 min(a, k) + max(a, k) + 1
        double* blk = env.data() + 49 * (size_t)(L.row_off[r] + r - L.first[r]);
        for (int a = 0; a < 7; a++)
            for (int k = 0; k < a; k++) blk[7 * a + k] = blk[7 * k + a];
    }
    vba_host::expand_envelope(L, env.data(), H.data());
    printf("expand n_free %d first", L.n_free);
    for (int v : L.first) printf(" %d", v);
    printf(" H");
    for (double v : H) printf(" %.0f", v);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc > 2 && !strcmp(argv[1], "--call")) { one_call(argc - 2, argv + 2); return 0; }
    if (argc > 2 && !strcmp(argv[1], "--expand")) { expand(argv[2]); return 0; }
    for (int a = 1; a < argc; a++) {
        Graph G;
        if (!G.load(argv[a])) { printf("error load\n"); continue; }
        const vba_posegraph_problem& P = G.P;
        vba_host::PoseGraphLayout L;
        std::string err;
        if (vba_host::build_posegraph(&P, L, err, (long long)G.env_before)) { printf("error %s\n", err.c_str()); continue; }
        if (const char* bad = invariants(P, L)) { printf("error invariant: %s\n", bad); continue; }
        int widest = 0;
        for (int r = 0; r < L.n_free; r++) widest = std::max(widest, r - L.first[r] + 1);
        printf("ok n_free %d env %lld widest %d inc %zu pairs %zu pair_edges %zu\n", L.n_free, L.env_blocks, widest, L.inc.size(), L.pair_lo.size(),
               L.pair_edge.size());
    }
    return 0;
}
