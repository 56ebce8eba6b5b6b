// Sanitizer harness of the host half of vba_search_triangulation (mc_slam_amd/csrc/vba_host_search_tri.h, vba_host_arena.h): plain
// C++, built by tests/test_host_search_tri.py with g++ -fsanitize=address,undefined.
//   host_search_tri_check <file>...     one line per file: "ok key value ..." or "error <message>"
// SearchTriCall (with the node join) runs as the library's driver runs it (run_call, tests/host_check.h); every array of the
// callers is a heap block of its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as
// an offset into the arena.  sum_query runs over the used query slots of all pairs, one after the other.
// Files (little-endian, written by the test): i32 n, then per pair i32 hd[15] = n_keys1 len1 n_keys2 len2 n_nodes1 nn1 nf1 n_nodes2
// nn2 nf2 n_levels2 lv th_low check_orientation nulls, f64 c[13] (F12 epipole chi2_epi epipole_r2), then per side u8 desc[len][32]
// has_mp[len], f64 uv[len][2], f32 angle[len], u32 node_id[nn], i32 node_begin[nn + 1] node_feat[nf], after side 2
// u8 oct2[len2], f64 sigma2[lv] scale[lv].  n_keys / n_nodes / n_levels2 are the fields, len / nn / lv the arrays; nulls: 1 desc2, 2 state,
// 4 the problem, 8 scale_2, 16 the result, 32 pairs, 64 angle1, 128 node_begin1, 256 node_id2, 512 node_feat2, 1024 has_mp1,
// 2048 oct2
#include "../mc_slam_amd/csrc/vba_host_search_tri.h"

#include "host_check.h"

using namespace vba_host;

static void st_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_search_tri_problem> P(ok ? n : 0);
    std::vector<vba_search_tri_result> R(P.size());
    std::vector<vba_search_tri_problem*> pp(P.size());
    std::vector<vba_search_tri_result*> rr(P.size());
    std::vector<size_t> len1(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[15];
        double c[13];
        ok = fread(hd, 4, 15, f) == 15 && fread(c, 8, 13, f) == 13 && hd[1] >= 0 && hd[3] >= 0 && hd[5] >= 0 && hd[6] >= 0 && hd[8] >= 0 && hd[9] >= 0 && hd[11] >= 0;
        if (!ok) break;
        vba_search_tri_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        const size_t l1 = hd[1], l2 = hd[3];
        len1[k] = l1;
        p.n_keys1 = hd[0]; p.n_keys2 = hd[2]; p.n_nodes1 = hd[4]; p.n_nodes2 = hd[7]; p.n_levels2 = hd[10]; p.th_low = hd[12]; p.check_orientation = hd[13];
        std::memcpy(p.F12, c, 72); p.epipole[0] = c[9]; p.epipole[1] = c[10]; p.chi2_epi = c[11]; p.epipole_r2 = c[12];
        p.desc1 = H.read<uint8_t>(f, 32 * l1, ok); p.has_mp1 = H.read<uint8_t>(f, l1, ok); p.uv1 = H.read<double>(f, 2 * l1, ok); p.angle1 = H.read<float>(f, l1, ok);
        p.node_id1 = H.read<uint32_t>(f, hd[5], ok); p.node_begin1 = H.read<int32_t>(f, hd[5] + 1, ok); p.node_feat1 = H.read<int32_t>(f, hd[6], ok);
        p.desc2 = H.read<uint8_t>(f, 32 * l2, ok); p.has_mp2 = H.read<uint8_t>(f, l2, ok); p.uv2 = H.read<double>(f, 2 * l2, ok); p.angle2 = H.read<float>(f, l2, ok);
        p.node_id2 = H.read<uint32_t>(f, hd[8], ok); p.node_begin2 = H.read<int32_t>(f, hd[8] + 1, ok); p.node_feat2 = H.read<int32_t>(f, hd[9], ok);
        p.oct2 = H.read<uint8_t>(f, l2, ok);
        p.level_sigma2_2 = H.read<double>(f, hd[11], ok); p.scale_2 = H.read<double>(f, hd[11], ok);
        R[k].match12 = H.get<int32_t>(l1); R[k].best_dist = H.get<uint8_t>(l1); R[k].state = H.get<uint8_t>(l1); R[k].pairs = H.get<int32_t>(2 * l1);
        R[k].status = -7; R[k].n_matches = -7;
        const int nl = hd[14];
        if (nl & 1) p.desc2 = nullptr;
        if (nl & 2) R[k].state = nullptr;
        if (nl & 8) p.scale_2 = nullptr;
        if (nl & 32) R[k].pairs = nullptr;
        if (nl & 64) p.angle1 = nullptr;
        if (nl & 128) p.node_begin1 = nullptr;
        if (nl & 256) p.node_id2 = nullptr;
        if (nl & 512) p.node_feat2 = nullptr;
        if (nl & 1024) p.has_mp1 = nullptr;
        if (nl & 2048) p.oct2 = nullptr;
        pp[k] = (nl & 4) ? nullptr : &p;
        rr[k] = (nl & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    SearchTriCall C;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const StBatch& B, void* hin) {
        const StDesc* desc = at<StDesc>(hin, C.A.desc);
        printf("ok k1 %zu k2 %zu feat_tot %zu lev_tot %zu upload %zu back %zu total %zu desc %zu key1 %zu key2 %zu query %zu feat %zu lev %zu out %zu match12 %zu best_dist %zu state %zu",
               C.T.k1, C.T.k2, C.T.feat, C.T.lev, C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.A.desc, C.A.key1, C.A.key2, C.A.query, C.A.feat, C.A.lev, C.A.out, C.A.match12,
               C.A.best_dist, C.A.state);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, key1); PRINT_BIND(B, hin, key2); PRINT_BIND(B, hin, query); PRINT_BIND(B, hin, feat); PRINT_BIND(B, hin, lev);
        PRINT_BIND(B, hin, out); PRINT_BIND(B, hin, match12); PRINT_BIND(B, hin, best_dist); PRINT_BIND(B, hin, state);
        unsigned long long sq = 0, pos = 0;
        long long nq = 0;
        for (int k = 0; k < n; k++) {
            sq += checksum(at<StQuery>(hin, C.A.query) + desc[k].key1_0, sizeof(StQuery) * (size_t)desc[k].n_q, &pos);
            nq += desc[k].n_q;
        }
        printf(" n_q %lld sum_query %llu sum_desc %llu sum_key1 %llu sum_key2 %llu sum_feat %llu sum_lev %llu", nq, sq, checksum(desc, sizeof(StDesc) * n),
               checksum(at<char>(hin, C.A.key1), sizeof(StKey) * C.T.k1), checksum(at<char>(hin, C.A.key2), sizeof(StKey) * C.T.k2), checksum(at<char>(hin, C.A.feat), 4 * C.T.feat),
               checksum(at<char>(hin, C.A.lev), 8 * C.T.lev));
    }, [&](void* hout) {
        // what came back: keypoint i of the call has match12 = i mod 5 - 1 (-1 for every fifth), best_dist = i mod 251, state = i mod 5; pair k
        // reports hist[b] = k + b, ind = (k, -1, k + 1), n_before_filter = 2 k, and n_matches = the entries >= 0 of its match12
        StOut* res = at<StOut>(hout, C.A.L.in_back(C.A.out));
        int32_t* m12 = at<int32_t>(hout, C.A.L.in_back(C.A.match12));
        unsigned char* bd = at<unsigned char>(hout, C.A.L.in_back(C.A.best_dist));
        unsigned char* st = at<unsigned char>(hout, C.A.L.in_back(C.A.state));
        for (size_t i = 0; i < C.T.k1; i++) { m12[i] = (int32_t)(i % 5) - 1; bd[i] = (unsigned char)(i % 251); st[i] = (unsigned char)(i % 5); }
        size_t key1_0 = 0;
        for (int k = 0; k < n; k++) {
            res[k].status = 0; res[k].n_before_filter = 2 * k; res[k].n_matches = 0;
            for (int i = 0; i < P[k].n_keys1; i++) res[k].n_matches += m12[key1_0 + i] >= 0;
            for (int b = 0; b < VBA_ST_HISTO; b++) res[k].hist[b] = k + b;
            res[k].ind[0] = k; res[k].ind[1] = -1; res[k].ind[2] = k + 1;
            key1_0 += (size_t)P[k].n_keys1;
        }
    });
    if (!ran) return;
    long long s_n = 0, s_status = 0, s_m12 = 0, s_bd = 0, s_st = 0, s_pairs = 0, s_hist = 0, s_ind = 0;
    for (int k = 0; k < n; k++) {
        s_n += R[k].n_matches * (long long)(k + 1) + R[k].n_before_filter;
        s_status += R[k].status;
        for (int b = 0; b < VBA_ST_HISTO; b++) s_hist += R[k].hist[b];
        s_ind += R[k].ind[0] + R[k].ind[1] + R[k].ind[2];
        for (size_t i = 0; i < len1[k] && (size_t)P[k].n_keys1 == len1[k]; i++) { s_m12 += R[k].match12[i]; s_bd += R[k].best_dist[i]; s_st += R[k].state[i]; }
        for (int j = 0; j < R[k].n_matches; j++) s_pairs += 3LL * R[k].pairs[2 * j] + R[k].pairs[2 * j + 1];
    }
    printf(" got_n %lld got_status %lld got_m12 %lld got_bd %lld got_st %lld got_pairs %lld got_hist %lld got_ind %lld\n", s_n, s_status, s_m12, s_bd, s_st,
           s_pairs, s_hist, s_ind);
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, st_file); }
