// Sanitizer harness of the host half of vba_search_for_initialization (mc_slam_amd/csrc/vba_host_search_init.h, vba_host_arena.h):
// plain C++, built by tests/test_host_search_init.py with g++ -fsanitize=address,undefined.
//   host_search_init_check <file>...     one line per file: "ok key value ..." or "error <message>"
// SearchInitCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of
// its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per pair i32 hd[11] = check_orientation th_low n_keys1 len1 n_keys2 len2
// grid_cols grid_rows len_cell len_feat nulls, f64 c[8] (bounds grid_inv_w grid_inv_h window_size nn_ratio), u8 desc1[len1][32]
// oct1[len1], f32 angle1[len1] prev_matched[len1][2], u8 desc2[len2][32], f64 uv2[len2][2], u8 oct2[len2], f32 angle2[len2],
// i32 cell_begin[len_cell] cell_feat[len_feat].  n_keys1 / n_keys2 are the fields, len1 / len2 the arrays.  Without
// check_orientation the angles are passed as NULL.  nulls: 1 desc1, 2 state, 4 the problem, 8 the result's prev_matched, 16 the
// result, 32 desc2, 64 cell_begin, 128 cell_feat, 256 match21, 512 angle1, 1024 angle2, 2048 matched_dist, 4096 uv2, 8192 oct1
#include "../mc_slam_amd/csrc/vba_host_search_init.h"

#include "host_check.h"

using namespace vba_host;

static void search_init_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_search_init_problem> P(ok ? n : 0);
    std::vector<vba_search_init_result> R(P.size());
    std::vector<vba_search_init_problem*> pp(P.size());
    std::vector<vba_search_init_result*> rr(P.size());
    std::vector<size_t> len1(P.size()), len2(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[11];
        double c[8];
        ok = fread(hd, 4, 11, f) == 11 && fread(c, 8, 8, f) == 8 && hd[3] >= 0 && hd[5] >= 0 && hd[8] >= 0 && hd[9] >= 0;
        if (!ok) break;
        vba_search_init_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        const size_t l1 = hd[3], l2 = hd[5];
        len1[k] = l1; len2[k] = l2;
        p.check_orientation = hd[0]; p.th_low = hd[1]; p.n_keys1 = hd[2]; p.n_keys2 = hd[4]; p.grid_cols = hd[6]; p.grid_rows = hd[7];
        std::memcpy(p.bounds, c, 32);
        p.grid_inv_w = c[4]; p.grid_inv_h = c[5]; p.window_size = c[6]; p.nn_ratio = (float)c[7];
        p.desc1 = H.read<uint8_t>(f, 32 * l1, ok); p.oct1 = H.read<uint8_t>(f, l1, ok); p.angle1 = H.read<float>(f, l1, ok);
        p.prev_matched = H.read<float>(f, 2 * l1, ok);
        p.desc2 = H.read<uint8_t>(f, 32 * l2, ok); p.uv2 = H.read<double>(f, 2 * l2, ok); p.oct2 = H.read<uint8_t>(f, l2, ok); p.angle2 = H.read<float>(f, l2, ok);
        p.cell_begin = H.read<int32_t>(f, hd[8], ok); p.cell_feat = H.read<int32_t>(f, hd[9], ok);
        if (!p.check_orientation) { p.angle1 = nullptr; p.angle2 = nullptr; }
        R[k].match12 = H.get<int32_t>(l1); R[k].best_idx = H.get<int32_t>(l1); R[k].best_dist = H.get<uint16_t>(l1); R[k].best_dist2 = H.get<uint16_t>(l1);
        R[k].bin = H.get<uint8_t>(l1); R[k].state = H.get<uint8_t>(l1); R[k].prev_matched = H.get<float>(2 * l1);
        R[k].match21 = H.get<int32_t>(l2); R[k].matched_dist = H.get<uint16_t>(l2);
        R[k].status = -7; R[k].n_matches = -7; R[k].n_before_filter = -7; R[k].n_stolen = -7; R[k].rounds = -7;
        const int nl = hd[10];
        if (nl & 1) p.desc1 = nullptr;
        if (nl & 2) R[k].state = nullptr;
        if (nl & 8) R[k].prev_matched = nullptr;
        if (nl & 32) p.desc2 = nullptr;
        if (nl & 64) p.cell_begin = nullptr;
        if (nl & 128) p.cell_feat = nullptr;
        if (nl & 256) R[k].match21 = nullptr;
        if (nl & 512) p.angle1 = nullptr;
        if (nl & 1024) p.angle2 = nullptr;
        if (nl & 2048) R[k].matched_dist = nullptr;
        if (nl & 4096) p.uv2 = nullptr;
        if (nl & 8192) p.oct1 = nullptr;
        pp[k] = (nl & 4) ? nullptr : &p;
        rr[k] = (nl & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    SearchInitCall C;
    void* staged = nullptr;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const SiBatch& B, void* hin) {
        staged = hin;
        printf("ok keys %zu qs %zu cells %zu feat_tot %zu max_keys %zu lds %zu grid %zu upload %zu back %zu total %zu desc %zu key %zu query %zu cell %zu feat %zu "
               "rounds %zu best_idx %zu best_dist %zu best_dist2 %zu state %zu next %zu cdist %zu",
               C.T.keys, C.T.qs, C.T.cells, C.T.feat, C.T.max_keys, C.lds_bytes(), C.grid(), C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.A.desc,
               C.A.key, C.A.query, C.A.cell, C.A.feat, C.A.rounds, C.A.best_idx, C.A.best_dist, C.A.best_dist2, C.A.state, C.A.next, C.A.cdist);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, key); PRINT_BIND(B, hin, query); PRINT_BIND(B, hin, cell_begin); PRINT_BIND(B, hin, cell_feat);
        PRINT_BIND(B, hin, rounds); PRINT_BIND(B, hin, best_idx); PRINT_BIND(B, hin, best_dist); PRINT_BIND(B, hin, best_dist2); PRINT_BIND(B, hin, state);
        PRINT_BIND(B, hin, next); PRINT_BIND(B, hin, cdist);
        printf(" sum_desc %llu sum_key %llu sum_query %llu sum_cell %llu sum_feat %llu", checksum(at<char>(hin, C.A.desc), sizeof(SiDesc) * n),
               checksum(at<char>(hin, C.A.key), sizeof(FuKey) * C.T.keys), checksum(at<char>(hin, C.A.query), sizeof(SiQuery) * C.T.qs),
               checksum(at<char>(hin, C.A.cell), 4 * C.T.cells), checksum(at<char>(hin, C.A.feat), 4 * C.T.feat));
    }, [&](void* hout) {
        // what came back: pair f ran f + 1 rounds; query i of the call (counted over all pairs), in a pair of nk keypoints in frame 2,
        // has best_idx = 5 i mod nk (-1 without keypoints), best_dist = i mod 257, best_dist2 = 3 i mod 257, state = 0 when i is a
        // multiple of 3 and nk > 0, else 2 + i mod 3
        auto back = [&](size_t off) { return C.A.L.in_back(off); };
        int32_t* rounds = at<int32_t>(hout, back(C.A.rounds));
        int32_t* bi = at<int32_t>(hout, back(C.A.best_idx));
        uint16_t* bd = at<uint16_t>(hout, back(C.A.best_dist));
        uint16_t* bd2 = at<uint16_t>(hout, back(C.A.best_dist2));
        unsigned char* st = at<unsigned char>(hout, back(C.A.state));
        const SiDesc* d = C.desc(staged);
        for (int k = 0; k < n; k++) {
            rounds[k] = k + 1;
            for (size_t i = (size_t)d[k].q0, e = i + (size_t)d[k].n_q; i < e; i++) {
                const size_t nk = (size_t)d[k].n_keys;
                bi[i] = nk ? (int32_t)((5 * i) % nk) : -1; bd[i] = (uint16_t)(i % 257); bd2[i] = (uint16_t)((3 * i) % 257);
                st[i] = (unsigned char)((i % 3 == 0 && nk) ? 0 : 2 + i % 3);
            }
        }
    });
    if (!ran) return;
    long long s_match = 0, s_before = 0, s_stolen = 0, s_status = 0, s_rounds = 0, s_m12 = 0, s_bi = 0, s_bd = 0, s_bd2 = 0, s_st = 0, s_bin = 0, s_m21 = 0, s_md = 0,
              s_hist = 0, s_ind = 0;
    double s_pm = 0;
    for (int k = 0; k < n; k++) {
        s_match += R[k].n_matches * (long long)(k + 1); s_before += R[k].n_before_filter * (long long)(k + 1); s_stolen += R[k].n_stolen * (long long)(k + 1);
        s_status += R[k].status; s_rounds += R[k].rounds * (long long)(k + 1);
        for (int b = 0; b < 30; b++) s_hist += R[k].hist[b] * (long long)(b + 1) * (k + 1);
        for (int b = 0; b < 3; b++) s_ind += R[k].ind[b] * (long long)(b + 1) * (k + 1);
        for (size_t i = 0; i < len1[k] && (size_t)P[k].n_keys1 == len1[k]; i++) {
            s_m12 += R[k].match12[i] * (long long)(i % 13 + 1); s_bi += R[k].best_idx[i]; s_bd += R[k].best_dist[i]; s_bd2 += R[k].best_dist2[i];
            s_st += R[k].state[i] * (long long)(i % 5 + 1); s_bin += R[k].bin[i] * (long long)(i % 7 + 1);
            s_pm += (double)R[k].prev_matched[2 * i] + 3 * (double)R[k].prev_matched[2 * i + 1];
        }
        for (size_t j = 0; j < len2[k] && (size_t)P[k].n_keys2 == len2[k]; j++) {
            s_m21 += R[k].match21[j] * (long long)(j % 11 + 1); s_md += R[k].matched_dist[j] * (long long)(j % 3 + 1);
        }
    }
    printf(" got_match %lld got_before %lld got_stolen %lld got_status %lld got_rounds %lld got_m12 %lld got_bi %lld got_bd %lld got_bd2 %lld got_st %lld got_bin %lld "
           "got_m21 %lld got_md %lld got_hist %lld got_ind %lld got_pm8 %lld\n",
           s_match, s_before, s_stolen, s_status, s_rounds, s_m12, s_bi, s_bd, s_bd2, s_st, s_bin, s_m21, s_md, s_hist, s_ind, (long long)(s_pm * 8));
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, search_init_file); }
