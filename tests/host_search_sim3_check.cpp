// Sanitizer harness of the host half of vba_search_by_sim3 (mc_slam_amd/csrc/vba_host_search_sim3.h, vba_host_arena.h): plain C++,
// built by tests/test_host_search_sim3.py with g++ -fsanitize=address,undefined.
//   host_search_sim3_check <file>...     one line per file: "ok key value ..." or "error <message>"
// SearchSim3Call runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of
// its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per pair i32 hd[2] = th_high nulls, f64 c[18] (K s12 R12 t12 th) and per
// keyframe i32 sh[8] = n_keys len_keys n_levels lv grid_cols grid_rows len_cell len_feat, f64 sc[19] (Rcw tcw bounds log_scale_factor
// grid_inv_w grid_inv_h), u8 desc[len_keys][32], f64 uv[len_keys][2], u8 oct[len_keys], f64 scale[lv], i32 cell_begin[len_cell]
// cell_feat[len_feat], u8 has_pt[len_keys] matched[len_keys], f64 pos[len_keys][3] dist_min[len_keys] dist_max[len_keys]
// pred_max[len_keys], u8 pt_desc[len_keys][32]; n_keys / n_levels are the fields, len_keys / lv the arrays.  nulls: 1 kf1.desc,
// 2 state1, 4 the problem, 8 kf2.scale, 16 the result, 32 best_dist2, 64 kf1.cell_begin, 128 kf2.cell_feat, 256 kf2.pos,
// 512 kf1.has_pt, 1024 kf2.oct, 2048 match12, 4096 kf1.matched, 8192 match2, 16384 level1.  After the pairs: i32 n_back and what
// "came back" for the call's queries in their packed order: i32 match[n_back], u16 best_dist[n_back], i8 level[n_back],
// u8 state[n_back]; n_back must be the call's number of queries.
#include "../mc_slam_amd/csrc/vba_host_search_sim3.h"

#include "host_check.h"

using namespace vba_host;

static bool read_kf(FILE* f, Heap& H, vba_search_sim3_kf& k, size_t& len) {
    int32_t sh[8];
    double sc[19];
    bool ok = fread(sh, 4, 8, f) == 8 && fread(sc, 8, 19, f) == 19 && sh[1] >= 0 && sh[3] >= 0 && sh[6] >= 0 && sh[7] >= 0;
    if (!ok) return false;
    std::memset(&k, 0, sizeof k);
    const size_t lk = sh[1];
    len = lk;
    k.n_keys = sh[0]; k.n_levels = sh[2]; k.grid_cols = sh[4]; k.grid_rows = sh[5];
    std::memcpy(k.Rcw, sc, 72); std::memcpy(k.tcw, sc + 9, 24); std::memcpy(k.bounds, sc + 12, 32);
    k.log_scale_factor = sc[16]; k.grid_inv_w = sc[17]; k.grid_inv_h = sc[18];
    k.desc = H.read<uint8_t>(f, 32 * lk, ok); k.uv = H.read<double>(f, 2 * lk, ok); k.oct = H.read<uint8_t>(f, lk, ok);
    k.scale = H.read<double>(f, sh[3], ok);
    k.cell_begin = H.read<int32_t>(f, sh[6], ok); k.cell_feat = H.read<int32_t>(f, sh[7], ok);
    k.has_pt = H.read<uint8_t>(f, lk, ok); k.matched = H.read<uint8_t>(f, lk, ok);
    k.pos = H.read<double>(f, 3 * lk, ok); k.dist_min = H.read<double>(f, lk, ok); k.dist_max = H.read<double>(f, lk, ok);
    k.pred_max = H.read<double>(f, lk, ok); k.pt_desc = H.read<uint8_t>(f, 32 * lk, ok);
    return ok;
}

static void search_sim3_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_search_sim3_problem> P(ok ? n : 0);
    std::vector<vba_search_sim3_result> R(P.size());
    std::vector<vba_search_sim3_problem*> pp(P.size());
    std::vector<vba_search_sim3_result*> rr(P.size());
    std::vector<size_t> len1(P.size()), len2(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[2];
        double c[18];
        ok = fread(hd, 4, 2, f) == 2 && fread(c, 8, 18, f) == 18;
        if (!ok) break;
        vba_search_sim3_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        ok = read_kf(f, H, p.kf1, len1[k]) && read_kf(f, H, p.kf2, len2[k]);
        if (!ok) break;
        std::memcpy(p.K, c, 32); p.s12 = c[4]; std::memcpy(p.R12, c + 5, 72); std::memcpy(p.t12, c + 14, 24); p.th = c[17];
        p.th_high = hd[0];
        vba_search_sim3_result& r = R[k];
        r.match1 = H.get<int32_t>(len1[k]); r.match2 = H.get<int32_t>(len2[k]); r.best_dist1 = H.get<uint16_t>(len1[k]); r.best_dist2 = H.get<uint16_t>(len2[k]);
        r.level1 = H.get<int8_t>(len1[k]); r.level2 = H.get<int8_t>(len2[k]); r.state1 = H.get<uint8_t>(len1[k]); r.state2 = H.get<uint8_t>(len2[k]);
        r.match12 = H.get<int32_t>(len1[k]);
        r.status = -7; r.n_found = -7;
        const int nl = hd[1];
        if (nl & 1) p.kf1.desc = nullptr;
        if (nl & 2) r.state1 = nullptr;
        if (nl & 8) p.kf2.scale = nullptr;
        if (nl & 32) r.best_dist2 = nullptr;
        if (nl & 64) p.kf1.cell_begin = nullptr;
        if (nl & 128) p.kf2.cell_feat = nullptr;
        if (nl & 256) p.kf2.pos = nullptr;
        if (nl & 512) p.kf1.has_pt = nullptr;
        if (nl & 1024) p.kf2.oct = nullptr;
        if (nl & 2048) r.match12 = nullptr;
        if (nl & 4096) p.kf1.matched = nullptr;
        if (nl & 8192) r.match2 = nullptr;
        if (nl & 16384) r.level1 = nullptr;
        pp[k] = (nl & 4) ? nullptr : &p;
        rr[k] = (nl & 16) ? nullptr : &r;
    }
    int32_t n_back = 0;
    ok = ok && fread(&n_back, 4, 1, f) == 1 && n_back >= 0;
    if (!ok) { printf("error load\n"); return; }
    const int32_t* b_match = H.read<int32_t>(f, n_back, ok);
    const uint16_t* b_dist = H.read<uint16_t>(f, n_back, ok);
    const int8_t* b_level = H.read<int8_t>(f, n_back, ok);
    const uint8_t* b_state = H.read<uint8_t>(f, n_back, ok);
    if (!ok) { printf("error load\n"); return; }
    SearchSim3Call C;
    bool back_ok = true;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const SsBatch& B, void* hin) {
        printf("ok keys %zu queries %zu cells %zu feat_tot %zu lev_tot %zu tiles %zu n_tiles %zu upload %zu back %zu total %zu dir %zu tile %zu key %zu query %zu cell %zu "
               "feat %zu lev %zu match %zu best_dist %zu level %zu state %zu",
               C.T.keys, C.T.queries, C.T.cells, C.T.feat, C.T.lev, C.T.tiles, C.grid(), C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.A.dir, C.A.tile,
               C.A.key, C.A.query, C.A.cell, C.A.feat, C.A.lev, C.A.match, C.A.best_dist, C.A.level, C.A.state);
        PRINT_BIND(B, hin, dir); PRINT_BIND(B, hin, tile); PRINT_BIND(B, hin, key); PRINT_BIND(B, hin, query); PRINT_BIND(B, hin, cell_begin);
        PRINT_BIND(B, hin, cell_feat); PRINT_BIND(B, hin, lev); PRINT_BIND(B, hin, match); PRINT_BIND(B, hin, best_dist); PRINT_BIND(B, hin, level);
        PRINT_BIND(B, hin, state);
        printf(" sum_dir %llu sum_tile %llu sum_key %llu sum_query %llu sum_cell %llu sum_feat %llu sum_lev %llu", checksum(at<char>(hin, C.A.dir), sizeof(SsDir) * 2 * n),
               checksum(at<char>(hin, C.A.tile), sizeof(SsTile) * C.T.tiles), checksum(at<char>(hin, C.A.key), sizeof(FuKey) * C.T.keys),
               checksum(at<char>(hin, C.A.query), sizeof(SsQuery) * C.T.queries), checksum(at<char>(hin, C.A.cell), 4 * C.T.cells),
               checksum(at<char>(hin, C.A.feat), 4 * C.T.feat), checksum(at<char>(hin, C.A.lev), 8 * C.T.lev));
    }, [&](void* hout) {
        back_ok = (size_t)n_back == C.T.queries;
        if (!back_ok) return;
        if (n_back) {
            std::memcpy(at<char>(hout, C.A.L.in_back(C.A.match)), b_match, 4 * (size_t)n_back);
            std::memcpy(at<char>(hout, C.A.L.in_back(C.A.best_dist)), b_dist, 2 * (size_t)n_back);
            std::memcpy(at<char>(hout, C.A.L.in_back(C.A.level)), b_level, (size_t)n_back);
            std::memcpy(at<char>(hout, C.A.L.in_back(C.A.state)), b_state, (size_t)n_back);
        }
    });
    if (!ran) return;
    if (!back_ok) { printf(" error n_back\n"); return; }
    // order-sensitive sums of what was written back: pair k, entry i of an array weighs (k + 1) * (i + 1); values are shifted to be positive
    unsigned long long s_found = 0, s_status = 0, s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < n; k++) {
        s_found += (unsigned long long)(R[k].n_found + 1) * (k + 1);
        s_status += (unsigned long long)R[k].status;
        const unsigned long long w = (unsigned long long)k + 1;
        for (size_t i = 0; i < len1[k] && (size_t)P[k].kf1.n_keys == len1[k]; i++) {
            s[0] += w * (i + 1) * (unsigned long long)(R[k].match1[i] + 2); s[1] += w * (i + 1) * R[k].best_dist1[i];
            s[2] += w * (i + 1) * (unsigned long long)(R[k].level1[i] + 129); s[3] += w * (i + 1) * R[k].state1[i];
            s[4] += w * (i + 1) * (unsigned long long)(R[k].match12[i] + 2);
        }
        for (size_t i = 0; i < len2[k] && (size_t)P[k].kf2.n_keys == len2[k]; i++) {
            s[5] += w * (i + 1) * (unsigned long long)(R[k].match2[i] + 2); s[6] += w * (i + 1) * R[k].best_dist2[i];
            s[7] += w * (i + 1) * (unsigned long long)(R[k].level2[i] + 129); s[8] += w * (i + 1) * R[k].state2[i];
        }
    }
    printf(" got_found %llu got_status %llu got_match1 %llu got_dist1 %llu got_level1 %llu got_state1 %llu got_match12 %llu got_match2 %llu got_dist2 %llu "
           "got_level2 %llu got_state2 %llu\n", s_found, s_status, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]);
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, search_sim3_file); }
