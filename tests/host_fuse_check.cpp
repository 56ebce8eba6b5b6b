// Sanitizer harness of the host half of vba_fuse (mc_slam_amd/csrc/vba_host_fuse.h, vba_host_arena.h): plain C++, built by
// tests/test_host_fuse.py with g++ -fsanitize=address,undefined.
//   host_fuse_check <file>...     one line per file: "ok key value ..." or "error <message>"
// FuseCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of its
// exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per problem i32 hd[13] = n_keys len_keys n_pt len_pt n_levels lv grid_cols
// grid_rows len_cell len_feat th_low check_reproj nulls, f64 c[29] (Rcw tcw Ow K bounds grid_inv_w grid_inv_h log_scale_factor th
// cos_view chi2_reproj), u8 desc[len_keys][32], f64 uv[len_keys][2], u8 oct[len_keys], f64 scale[lv] inv_level_sigma2[lv],
// i32 cell_begin[len_cell] cell_feat[len_feat], f64 pos[len_pt][3] normal[len_pt][3] dist_min[len_pt] dist_max[len_pt]
// pred_max[len_pt], u8 pt_desc[len_pt][32] skip[len_pt].  n_keys / n_pt / n_levels are the fields, len_* / lv the arrays; nulls: 1 desc,
// 2 state, 4 the problem, 8 scale, 16 the result, 32 best_dist, 64 cell_begin, 128 cell_feat, 256 pos, 512 skip, 1024 oct, 2048 uv of
// the result
#include "../mc_slam_amd/csrc/vba_host_fuse.h"

#include "host_check.h"

using namespace vba_host;

static void fuse_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_fuse_problem> P(ok ? n : 0);
    std::vector<vba_fuse_result> R(P.size());
    std::vector<vba_fuse_problem*> pp(P.size());
    std::vector<vba_fuse_result*> rr(P.size());
    std::vector<size_t> len_pt(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[13];
        double c[29];
        ok = fread(hd, 4, 13, f) == 13 && fread(c, 8, 29, f) == 29 && hd[1] >= 0 && hd[3] >= 0 && hd[5] >= 0 && hd[8] >= 0 && hd[9] >= 0;
        if (!ok) break;
        vba_fuse_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        const size_t lk = hd[1], lp = hd[3], lv = hd[5];
        len_pt[k] = lp;
        p.n_keys = hd[0]; p.n_pt = hd[2]; p.n_levels = hd[4]; p.grid_cols = hd[6]; p.grid_rows = hd[7]; p.th_low = hd[10]; p.check_reproj = hd[11];
        std::memcpy(p.Rcw, c, 72); std::memcpy(p.tcw, c + 9, 24); std::memcpy(p.Ow, c + 12, 24); std::memcpy(p.K, c + 15, 32); std::memcpy(p.bounds, c + 19, 32);
        p.grid_inv_w = c[23]; p.grid_inv_h = c[24]; p.log_scale_factor = c[25]; p.th = c[26]; p.cos_view = c[27]; p.chi2_reproj = c[28];
        p.desc = H.read<uint8_t>(f, 32 * lk, ok); p.uv = H.read<double>(f, 2 * lk, ok); p.oct = H.read<uint8_t>(f, lk, ok);
        p.scale = H.read<double>(f, lv, ok); p.inv_level_sigma2 = H.read<double>(f, lv, ok);
        p.cell_begin = H.read<int32_t>(f, hd[8], ok); p.cell_feat = H.read<int32_t>(f, hd[9], ok);
        p.pos = H.read<double>(f, 3 * lp, ok); p.normal = H.read<double>(f, 3 * lp, ok);
        p.dist_min = H.read<double>(f, lp, ok); p.dist_max = H.read<double>(f, lp, ok); p.pred_max = H.read<double>(f, lp, ok);
        p.pt_desc = H.read<uint8_t>(f, 32 * lp, ok); p.skip = H.read<uint8_t>(f, lp, ok);
        R[k].best_idx = H.get<int32_t>(lp); R[k].best_dist = H.get<uint16_t>(lp); R[k].level = H.get<int8_t>(lp); R[k].uv = H.get<double>(2 * lp);
        R[k].state = H.get<uint8_t>(lp);
        R[k].status = -7; R[k].n_found = -7;
        const int nl = hd[12];
        if (nl & 1) p.desc = nullptr;
        if (nl & 2) R[k].state = nullptr;
        if (nl & 8) p.scale = nullptr;
        if (nl & 32) R[k].best_dist = nullptr;
        if (nl & 64) p.cell_begin = nullptr;
        if (nl & 128) p.cell_feat = nullptr;
        if (nl & 256) p.pos = nullptr;
        if (nl & 512) p.skip = nullptr;
        if (nl & 1024) p.oct = nullptr;
        if (nl & 2048) R[k].uv = nullptr;
        pp[k] = (nl & 4) ? nullptr : &p;
        rr[k] = (nl & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    FuseCall C;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const FuBatch& B, void* hin) {
        printf("ok keys %zu pts %zu cells %zu feat_tot %zu lev_tot %zu tiles %zu n_tiles %zu upload %zu back %zu total %zu desc %zu tile %zu key %zu pt %zu cell %zu feat %zu lev %zu "
               "best_idx %zu best_dist %zu level %zu uv %zu state %zu",
               C.T.keys, C.T.pts, C.T.cells, C.T.feat, C.T.lev, C.T.tiles, C.grid(), C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.A.desc, C.A.tile, C.A.key, C.A.pt, C.A.cell,
               C.A.feat, C.A.lev, C.A.best_idx, C.A.best_dist, C.A.level, C.A.uv, C.A.state);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, tile); PRINT_BIND(B, hin, key); PRINT_BIND(B, hin, pt); PRINT_BIND(B, hin, cell_begin);
        PRINT_BIND(B, hin, cell_feat); PRINT_BIND(B, hin, lev); PRINT_BIND(B, hin, best_idx); PRINT_BIND(B, hin, best_dist); PRINT_BIND(B, hin, level);
        PRINT_BIND(B, hin, uv); PRINT_BIND(B, hin, state);
        printf(" sum_desc %llu sum_tile %llu sum_key %llu sum_pt %llu sum_cell %llu sum_feat %llu sum_lev %llu", checksum(at<char>(hin, C.A.desc), sizeof(FuDesc) * n),
               checksum(at<char>(hin, C.A.tile), sizeof(FuTile) * C.T.tiles), checksum(at<char>(hin, C.A.key), sizeof(FuKey) * C.T.keys),
               checksum(at<char>(hin, C.A.pt), sizeof(FuPoint) * C.T.pts), checksum(at<char>(hin, C.A.cell), 4 * C.T.cells), checksum(at<char>(hin, C.A.feat), 4 * C.T.feat),
               checksum(at<char>(hin, C.A.lev), 8 * C.T.lev));
    }, [&](void* hout) {
        // what came back: point i of the call has best_idx = i mod 7 - 1, best_dist = i mod 257, level = i mod 200 - 128, uv = (i / 4, -i / 8),
        // state = i mod 9
        int32_t* bi = at<int32_t>(hout, C.A.L.in_back(C.A.best_idx));
        uint16_t* bd = at<uint16_t>(hout, C.A.L.in_back(C.A.best_dist));
        int8_t* lv = at<int8_t>(hout, C.A.L.in_back(C.A.level));
        double* uv = at<double>(hout, C.A.L.in_back(C.A.uv));
        unsigned char* st = at<unsigned char>(hout, C.A.L.in_back(C.A.state));
        for (size_t i = 0; i < C.T.pts; i++) {
            bi[i] = (int32_t)(i % 7) - 1; bd[i] = (uint16_t)(i % 257); lv[i] = (int8_t)((int)(i % 200) - 128); uv[2 * i] = (double)i / 4; uv[2 * i + 1] = -(double)i / 8;
            st[i] = (unsigned char)(i % 9);
        }
    });
    if (!ran) return;
    long long s_found = 0, s_status = 0, s_bi = 0, s_bd = 0, s_lv = 0, s_st = 0;
    double s_uv = 0;
    for (int k = 0; k < n; k++) {
        s_found += R[k].n_found * (long long)(k + 1);
        s_status += R[k].status;
        for (size_t i = 0; i < len_pt[k] && (size_t)P[k].n_pt == len_pt[k]; i++) {
            s_bi += R[k].best_idx[i]; s_bd += R[k].best_dist[i]; s_lv += R[k].level[i]; s_st += R[k].state[i];
            s_uv += R[k].uv[2 * i] + 3 * R[k].uv[2 * i + 1];
        }
    }
    printf(" got_found %lld got_status %lld got_bi %lld got_bd %lld got_lv %lld got_st %lld got_uv8 %lld\n", s_found, s_status, s_bi, s_bd, s_lv, s_st,
           (long long)(s_uv * 8));
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, fuse_file); }
