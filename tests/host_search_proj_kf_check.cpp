// Sanitizer harness of the host half of vba_search_by_projection_kf (mc_slam_amd/csrc/vba_host_search_proj_kf.h, vba_host_arena.h):
// plain C++, built by tests/test_host_search_proj_kf.py with g++ -fsanitize=address,undefined.
//   host_search_proj_kf_check <file>...     one line per file: "ok key value ..." or "error <message>"
// SearchProjKfCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of
// its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per problem i32 hd[14] = mode check_orientation n_keys len_keys n_q len_q
// n_levels lv grid_cols grid_rows len_cell len_feat th_dist nulls, f64 c[28] (Rcw tcw Ow K bounds grid_inv_w grid_inv_h
// log_scale_factor th cos_view), u8 desc[len_keys][32], f64 uv[len_keys][2], u8 oct[len_keys], f32 angle[len_keys],
// u8 occupied[len_keys], f64 scale[lv], i32 cell_begin[len_cell] cell_feat[len_feat], f64 q_pos[len_q][3], u8 q_desc[len_q][32]
// q_skip[len_q], f32 q_angle[len_q], f64 q_normal[len_q][3] q_dist_min[len_q] q_dist_max[len_q] q_pred_max[len_q].  n_keys / n_q /
// n_levels are the fields, len_* / lv the arrays.  The arrays the mode does not read are passed as NULL (q_normal in reloc mode; angle
// and q_angle in loop mode and without check_orientation).  nulls: 1 desc, 2 state, 4 the problem, 8 scale, 16 the result, 32 level,
// 64 cell_begin, 128 cell_feat, 256 q_pos, 512 q_dist_max, 1024 occupied, 2048 key_match, 4096 q_normal, 8192 angle, 16384 q_angle,
// 32768 bin
#include "../mc_slam_amd/csrc/vba_host_search_proj_kf.h"

#include "host_check.h"

using namespace vba_host;

static void search_proj_kf_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_search_proj_kf_problem> P(ok ? n : 0);
    std::vector<vba_search_proj_kf_result> R(P.size());
    std::vector<vba_search_proj_kf_problem*> pp(P.size());
    std::vector<vba_search_proj_kf_result*> rr(P.size());
    std::vector<size_t> len_q(P.size()), len_k(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[14];
        double c[28];
        ok = fread(hd, 4, 14, f) == 14 && fread(c, 8, 28, f) == 28 && hd[3] >= 0 && hd[5] >= 0 && hd[7] >= 0 && hd[10] >= 0 && hd[11] >= 0;
        if (!ok) break;
        vba_search_proj_kf_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        const size_t lk = hd[3], lq = hd[5], lv = hd[7];
        len_k[k] = lk; len_q[k] = lq;
        p.mode = hd[0]; p.check_orientation = hd[1]; p.n_keys = hd[2]; p.n_q = hd[4]; p.n_levels = hd[6]; p.grid_cols = hd[8]; p.grid_rows = hd[9];
        p.th_dist = hd[12];
        std::memcpy(p.Rcw, c, 72); std::memcpy(p.tcw, c + 9, 24); std::memcpy(p.Ow, c + 12, 24); std::memcpy(p.K, c + 15, 32); std::memcpy(p.bounds, c + 19, 32);
        p.grid_inv_w = c[23]; p.grid_inv_h = c[24]; p.log_scale_factor = c[25]; p.th = c[26]; p.cos_view = c[27];
        p.desc = H.read<uint8_t>(f, 32 * lk, ok); p.uv = H.read<double>(f, 2 * lk, ok); p.oct = H.read<uint8_t>(f, lk, ok);
        p.angle = H.read<float>(f, lk, ok); p.occupied = H.read<uint8_t>(f, lk, ok); p.scale = H.read<double>(f, lv, ok);
        p.cell_begin = H.read<int32_t>(f, hd[10], ok); p.cell_feat = H.read<int32_t>(f, hd[11], ok);
        p.q_pos = H.read<double>(f, 3 * lq, ok); p.q_desc = H.read<uint8_t>(f, 32 * lq, ok); p.q_skip = H.read<uint8_t>(f, lq, ok);
        p.q_angle = H.read<float>(f, lq, ok);
        p.q_normal = H.read<double>(f, 3 * lq, ok); p.q_dist_min = H.read<double>(f, lq, ok); p.q_dist_max = H.read<double>(f, lq, ok);
        p.q_pred_max = H.read<double>(f, lq, ok);
        const bool reloc = p.mode == VBA_SEARCH_PROJ_KF_RELOC;
        if (reloc) p.q_normal = nullptr;
        if (!reloc || !p.check_orientation) { p.q_angle = nullptr; p.angle = nullptr; }
        R[k].best_idx = H.get<int32_t>(lq); R[k].best_dist = H.get<uint16_t>(lq); R[k].level = H.get<int8_t>(lq);
        R[k].uv = H.get<double>(2 * lq); R[k].bin = H.get<uint8_t>(lq); R[k].state = H.get<uint8_t>(lq);
        R[k].key_match = H.get<int32_t>(lk);
        R[k].status = -7; R[k].n_matches = -7; R[k].n_before_filter = -7; R[k].rounds = -7;
        const int nl = hd[13];
        if (nl & 1) p.desc = nullptr;
        if (nl & 2) R[k].state = nullptr;
        if (nl & 8) p.scale = nullptr;
        if (nl & 32) R[k].level = nullptr;
        if (nl & 64) p.cell_begin = nullptr;
        if (nl & 128) p.cell_feat = nullptr;
        if (nl & 256) p.q_pos = nullptr;
        if (nl & 512) p.q_dist_max = nullptr;
        if (nl & 1024) p.occupied = nullptr;
        if (nl & 2048) R[k].key_match = nullptr;
        if (nl & 4096) p.q_normal = nullptr;
        if (nl & 8192) p.angle = nullptr;
        if (nl & 16384) p.q_angle = nullptr;
        if (nl & 32768) R[k].bin = nullptr;
        pp[k] = (nl & 4) ? nullptr : &p;
        rr[k] = (nl & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    SearchProjKfCall C;
    void* staged = nullptr;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const SkBatch& B, void* hin) {
        staged = hin;
        printf("ok keys %zu qs %zu cells %zu feat_tot %zu lev_tot %zu max_keys %zu lds %zu grid %zu upload %zu back %zu total %zu desc %zu key %zu occupied %zu query %zu "
               "cell %zu feat %zu lev %zu rounds %zu best_idx %zu best_dist %zu level %zu uv %zu state %zu rad %zu prev %zu",
               C.T.keys, C.T.qs, C.T.cells, C.T.feat, C.T.lev, C.T.max_keys, C.lds_bytes(), C.grid(), C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(),
               C.A.desc, C.A.key, C.A.occupied, C.A.query, C.A.cell, C.A.feat, C.A.lev, C.A.rounds, C.A.best_idx, C.A.best_dist, C.A.level, C.A.uv, C.A.state,
               C.A.rad, C.A.prev);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, key); PRINT_BIND(B, hin, occupied); PRINT_BIND(B, hin, query); PRINT_BIND(B, hin, cell_begin);
        PRINT_BIND(B, hin, cell_feat); PRINT_BIND(B, hin, lev); PRINT_BIND(B, hin, rounds); PRINT_BIND(B, hin, best_idx); PRINT_BIND(B, hin, best_dist);
        PRINT_BIND(B, hin, level); PRINT_BIND(B, hin, uv); PRINT_BIND(B, hin, state); PRINT_BIND(B, hin, rad); PRINT_BIND(B, hin, prev);
        printf(" sum_desc %llu sum_key %llu sum_occ %llu sum_query %llu sum_cell %llu sum_feat %llu sum_lev %llu", checksum(at<char>(hin, C.A.desc), sizeof(SpDesc) * n),
               checksum(at<char>(hin, C.A.key), sizeof(FuKey) * C.T.keys), checksum(at<char>(hin, C.A.occupied), C.T.keys),
               checksum(at<char>(hin, C.A.query), sizeof(SpQuery) * C.T.qs), checksum(at<char>(hin, C.A.cell), 4 * C.T.cells),
               checksum(at<char>(hin, C.A.feat), 4 * C.T.feat), checksum(at<char>(hin, C.A.lev), 8 * C.T.lev));
    }, [&](void* hout) {
        // what came back: problem f ran f + 1 rounds; query i of the call (counted over all problems), in a problem of nk keypoints, has
        // best_idx = 5 i mod nk (-1 without keypoints), best_dist = i mod 257, level = i mod 200 - 128, uv = (i / 4, -i / 8),
        // state = 0 when i is a multiple of 3 and nk > 0, else 1 + i mod 8
        auto back = [&](size_t off) { return C.A.L.in_back(off); };
        int32_t* rounds = at<int32_t>(hout, back(C.A.rounds));
        int32_t* bi = at<int32_t>(hout, back(C.A.best_idx));
        uint16_t* bd = at<uint16_t>(hout, back(C.A.best_dist));
        int8_t* lv = at<int8_t>(hout, back(C.A.level));
        double* uv = at<double>(hout, back(C.A.uv));
        unsigned char* st = at<unsigned char>(hout, back(C.A.state));
        const SpDesc* d = C.desc(staged);
        for (int k = 0; k < n; k++) {
            rounds[k] = k + 1;
            for (size_t i = (size_t)d[k].q0, e = i + (size_t)d[k].n_q; i < e; i++) {
                const size_t nk = (size_t)d[k].n_keys;
                bi[i] = nk ? (int32_t)((5 * i) % nk) : -1; bd[i] = (uint16_t)(i % 257);
                lv[i] = (int8_t)((int)(i % 200) - 128); uv[2 * i] = (double)i / 4; uv[2 * i + 1] = -(double)i / 8;
                st[i] = (unsigned char)((i % 3 == 0 && nk) ? 0 : 1 + i % 8);
            }
        }
    });
    if (!ran) return;
    long long s_match = 0, s_before = 0, s_status = 0, s_rounds = 0, s_bi = 0, s_bd = 0, s_lv = 0, s_st = 0, s_bin = 0, s_km = 0, s_hist = 0, s_ind = 0;
    double s_uv = 0;
    for (int k = 0; k < n; k++) {
        s_match += R[k].n_matches * (long long)(k + 1); s_before += R[k].n_before_filter * (long long)(k + 1);
        s_status += R[k].status; s_rounds += R[k].rounds * (long long)(k + 1);
        for (int b = 0; b < 30; b++) s_hist += R[k].hist[b] * (long long)(b + 1) * (k + 1);
        for (int b = 0; b < 3; b++) s_ind += R[k].ind[b] * (long long)(b + 1) * (k + 1);
        for (size_t i = 0; i < len_q[k] && (size_t)P[k].n_q == len_q[k]; i++) {
            s_bi += R[k].best_idx[i]; s_bd += R[k].best_dist[i]; s_lv += R[k].level[i]; s_st += R[k].state[i] * (long long)(i % 5 + 1);
            s_bin += R[k].bin[i] * (long long)(i % 7 + 1);
            s_uv += R[k].uv[2 * i] + 3 * R[k].uv[2 * i + 1];
        }
        for (size_t j = 0; j < len_k[k] && (size_t)P[k].n_keys == len_k[k]; j++) s_km += R[k].key_match[j] * (long long)(j % 11 + 1);
    }
    printf(" got_match %lld got_before %lld got_status %lld got_rounds %lld got_bi %lld got_bd %lld got_lv %lld got_st %lld got_bin %lld got_km %lld "
           "got_hist %lld got_ind %lld got_uv8 %lld\n",
           s_match, s_before, s_status, s_rounds, s_bi, s_bd, s_lv, s_st, s_bin, s_km, s_hist, s_ind, (long long)(s_uv * 8));
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, search_proj_kf_file); }
