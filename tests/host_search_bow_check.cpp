// Sanitizer harness of the host half of vba_search_by_bow (mc_slam_amd/csrc/vba_host_search_bow.h, vba_host_arena.h): plain C++,
// built by tests/test_host_search_bow.py with g++ -fsanitize=address,undefined.
//   host_search_bow_check <file>...     one line per file: "ok key value ..." or "error <message>"
// SearchBowCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of
// its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per pair i32 hd[14] = mode check_orientation th_low n_keys1 len1 n_keys2
// len2 n_nodes1 len_nodes1 n_nodes2 len_nodes2 len_feat1 len_feat2 nulls, f32 nn_ratio, u8 desc1[len1][32] desc2[len2][32]
// good_mp1[len1] good_mp2[len2], f32 angle1[len1] angle2[len2], u32 node_id1[len_nodes1], i32 node_begin1[len_nodes1 + 1]
// node_feat1[len_feat1], u32 node_id2[len_nodes2], i32 node_begin2[len_nodes2 + 1] node_feat2[len_feat2].  n_keys / n_nodes are the
// fields, len_* the arrays.  good_mp2 is passed as NULL in KF_FRAME mode, the angles without check_orientation.  nulls: 1 desc1,
// 2 state, 4 the problem, 8 desc2, 16 the result, 32 best_dist2, 64 node_begin1, 128 node_feat2, 256 good_mp1, 512 good_mp2,
// 1024 match21, 2048 match12, 4096 angle1, 8192 angle2, 16384 node_id2, 32768 bin
#include "../mc_slam_amd/csrc/vba_host_search_bow.h"

#include "host_check.h"

using namespace vba_host;

static void search_bow_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_search_bow_problem> P(ok ? n : 0);
    std::vector<vba_search_bow_result> R(P.size());
    std::vector<vba_search_bow_problem*> pp(P.size());
    std::vector<vba_search_bow_result*> rr(P.size());
    std::vector<size_t> len1(P.size()), len2(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[14];
        float ratio;
        ok = fread(hd, 4, 14, f) == 14 && fread(&ratio, 4, 1, f) == 1 && hd[4] >= 0 && hd[6] >= 0 && hd[8] >= 0 && hd[10] >= 0 && hd[11] >= 0 && hd[12] >= 0;
        if (!ok) break;
        vba_search_bow_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        const size_t l1 = hd[4], l2 = hd[6];
        len1[k] = l1; len2[k] = l2;
        p.mode = hd[0]; p.check_orientation = hd[1]; p.th_low = hd[2]; p.nn_ratio = ratio; p.n_keys1 = hd[3]; p.n_keys2 = hd[5];
        p.n_nodes1 = hd[7]; p.n_nodes2 = hd[9];
        p.desc1 = H.read<uint8_t>(f, 32 * l1, ok); p.desc2 = H.read<uint8_t>(f, 32 * l2, ok);
        p.good_mp1 = H.read<uint8_t>(f, l1, ok); p.good_mp2 = H.read<uint8_t>(f, l2, ok);
        p.angle1 = H.read<float>(f, l1, ok); p.angle2 = H.read<float>(f, l2, ok);
        p.node_id1 = H.read<uint32_t>(f, hd[8], ok); p.node_begin1 = H.read<int32_t>(f, (size_t)hd[8] + 1, ok); p.node_feat1 = H.read<int32_t>(f, hd[11], ok);
        p.node_id2 = H.read<uint32_t>(f, hd[10], ok); p.node_begin2 = H.read<int32_t>(f, (size_t)hd[10] + 1, ok); p.node_feat2 = H.read<int32_t>(f, hd[12], ok);
        if (p.mode == VBA_SEARCH_BOW_KF_FRAME) p.good_mp2 = nullptr;
        if (!p.check_orientation) { p.angle1 = nullptr; p.angle2 = nullptr; }
        R[k].match12 = H.get<int32_t>(l1); R[k].best_idx = H.get<int32_t>(l1); R[k].best_dist = H.get<uint16_t>(l1); R[k].best_dist2 = H.get<uint16_t>(l1);
        R[k].bin = H.get<uint8_t>(l1); R[k].state = H.get<uint8_t>(l1); R[k].match21 = H.get<int32_t>(l2);
        R[k].status = -7; R[k].n_matches = -7; R[k].n_before_filter = -7; R[k].rounds = -7;
        const int nl = hd[13];
        if (nl & 1) p.desc1 = nullptr;
        if (nl & 2) R[k].state = nullptr;
        if (nl & 8) p.desc2 = nullptr;
        if (nl & 32) R[k].best_dist2 = nullptr;
        if (nl & 64) p.node_begin1 = nullptr;
        if (nl & 128) p.node_feat2 = nullptr;
        if (nl & 256) p.good_mp1 = nullptr;
        if (nl & 512) p.good_mp2 = nullptr;
        if (nl & 1024) R[k].match21 = nullptr;
        if (nl & 2048) R[k].match12 = nullptr;
        if (nl & 4096) p.angle1 = nullptr;
        if (nl & 8192) p.angle2 = nullptr;
        if (nl & 16384) p.node_id2 = nullptr;
        if (nl & 32768) R[k].bin = nullptr;
        pp[k] = (nl & 4) ? nullptr : &p;
        rr[k] = (nl & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    SearchBowCall C;
    void* staged = nullptr;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const SbBatch& B, void* hin) {
        staged = hin;
        printf("ok k1 %zu k2 %zu feat_tot %zu max_keys2 %zu lds %zu grid %zu upload %zu back %zu total %zu desc %zu key1 %zu key2 %zu role %zu blocked %zu query %zu "
               "feat %zu rounds %zu best_idx %zu best_dist %zu best_dist2 %zu state %zu prev %zu",
               C.T.k1, C.T.k2, C.T.feat, C.T.max_keys2, C.lds_bytes(), C.grid(), C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.A.desc, C.A.key1,
               C.A.key2, C.A.role, C.A.blocked, C.A.query, C.A.feat, C.A.rounds, C.A.best_idx, C.A.best_dist, C.A.best_dist2, C.A.state, C.A.prev);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, key1); PRINT_BIND(B, hin, key2); PRINT_BIND(B, hin, role); PRINT_BIND(B, hin, blocked);
        PRINT_BIND(B, hin, query); PRINT_BIND(B, hin, feat); PRINT_BIND(B, hin, rounds); PRINT_BIND(B, hin, best_idx); PRINT_BIND(B, hin, best_dist);
        PRINT_BIND(B, hin, best_dist2); PRINT_BIND(B, hin, state); PRINT_BIND(B, hin, prev);
        // a pair uses the first n_q of its query slots: the payload is those of all pairs, back to back
        const SbDesc* d = C.desc(hin);
        unsigned long long sq = 0, pos = 0, nq = 0;
        for (int k = 0; k < n; k++) {
            sq += checksum(at<SbQuery>(hin, C.A.query) + d[k].key1_0, sizeof(SbQuery) * (size_t)d[k].n_q, &pos);
            nq += (unsigned long long)d[k].n_q;
        }
        printf(" n_q %llu sum_desc %llu sum_key1 %llu sum_key2 %llu sum_role %llu sum_blocked %llu sum_query %llu sum_feat %llu", nq,
               checksum(at<char>(hin, C.A.desc), sizeof(SbDesc) * n), checksum(at<char>(hin, C.A.key1), sizeof(SbKey) * C.T.k1),
               checksum(at<char>(hin, C.A.key2), sizeof(SbKey) * C.T.k2), checksum(at<char>(hin, C.A.role), C.T.k1), checksum(at<char>(hin, C.A.blocked), C.T.k2), sq,
               checksum(at<char>(hin, C.A.feat), 4 * C.T.feat));
    }, [&](void* hout) {
        // what came back: pair k ran k + 1 rounds; keypoint i of side 1 of the call (counted over all pairs), in a pair of n2 keypoints on
        // side 2, keeps the state of its role when that is not 0; a query has best_idx = 5 i mod n2 (-1 without keypoints),
        // best_dist = i mod 257, best_dist2 = 3 i mod 257, state = 0 when i is a multiple of 3 and n2 > 0, else 3 + i mod 2
        auto back = [&](size_t off) { return C.A.L.in_back(off); };
        int32_t* rounds = at<int32_t>(hout, back(C.A.rounds));
        int32_t* bi = at<int32_t>(hout, back(C.A.best_idx));
        uint16_t* bd = at<uint16_t>(hout, back(C.A.best_dist));
        uint16_t* bd2 = at<uint16_t>(hout, back(C.A.best_dist2));
        unsigned char* st = at<unsigned char>(hout, back(C.A.state));
        const SbDesc* d = C.desc(staged);
        const unsigned char* role = at<unsigned char>(staged, C.A.role);
        for (int k = 0; k < n; k++) {
            rounds[k] = k + 1;
            const size_t n2 = (size_t)d[k].n_keys2;
            for (size_t i = (size_t)d[k].key1_0, e = i + (size_t)d[k].n_keys1; i < e; i++) {
                if (role[i] != 0) { bi[i] = -1; bd[i] = 256; bd2[i] = 256; st[i] = role[i]; continue; }
                bi[i] = n2 ? (int32_t)((5 * i) % n2) : -1; bd[i] = (uint16_t)(i % 257); bd2[i] = (uint16_t)((3 * i) % 257);
                st[i] = (unsigned char)((i % 3 == 0 && n2) ? 0 : 3 + i % 2);
            }
        }
    });
    if (!ran) return;
    long long s_match = 0, s_before = 0, s_status = 0, s_rounds = 0, s_m12 = 0, s_bi = 0, s_bd = 0, s_bd2 = 0, s_st = 0, s_bin = 0, s_m21 = 0, s_hist = 0, s_ind = 0;
    for (int k = 0; k < n; k++) {
        s_match += R[k].n_matches * (long long)(k + 1); s_before += R[k].n_before_filter * (long long)(k + 1);
        s_status += R[k].status; s_rounds += R[k].rounds * (long long)(k + 1);
        for (int b = 0; b < 30; b++) s_hist += R[k].hist[b] * (long long)(b + 1) * (k + 1);
        for (int b = 0; b < 3; b++) s_ind += R[k].ind[b] * (long long)(b + 1) * (k + 1);
        for (size_t i = 0; i < len1[k] && (size_t)P[k].n_keys1 == len1[k]; i++) {
            s_m12 += R[k].match12[i] * (long long)(i % 13 + 1); s_bi += R[k].best_idx[i]; s_bd += R[k].best_dist[i]; s_bd2 += R[k].best_dist2[i];
            s_st += R[k].state[i] * (long long)(i % 5 + 1); s_bin += R[k].bin[i] * (long long)(i % 7 + 1);
        }
        for (size_t j = 0; j < len2[k] && (size_t)P[k].n_keys2 == len2[k]; j++) s_m21 += R[k].match21[j] * (long long)(j % 11 + 1);
    }
    printf(" got_match %lld got_before %lld got_status %lld got_rounds %lld got_m12 %lld got_bi %lld got_bd %lld got_bd2 %lld got_st %lld got_bin %lld got_m21 %lld "
           "got_hist %lld got_ind %lld\n",
           s_match, s_before, s_status, s_rounds, s_m12, s_bi, s_bd, s_bd2, s_st, s_bin, s_m21, s_hist, s_ind);
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, search_bow_file); }
