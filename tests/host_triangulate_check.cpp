// Sanitizer harness of the host half of vba_triangulate (mc_slam_amd/csrc/vba_host_triangulate.h, vba_host_arena.h): plain C++,
// built by tests/test_host_triangulate.py with g++ -fsanitize=address,undefined.
//   host_triangulate_check <file>...     one line per file: "ok key value ..." or "error <message>"
// TriCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of its
// exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per pair i32 n_matches len n_levels1 lv1 n_levels2 lv2 nulls,
// f64 c[41] (Rcw1 tcw1 Ow1 K1 Rcw2 tcw2 Ow2 K2 ratio_factor cos_max chi2_th), f64 sigma2_1[lv1] scale_1[lv1] sigma2_2[lv2]
// scale_2[lv2], f64 uv1[len][2] uv2[len][2], u8 oct1[len] oct2[len].  n_matches / n_levels are the fields, len / lv the arrays;
// nulls: 1 uv2 = NULL, 2 reason = NULL, 4 the problem itself is NULL, 8 scale_2 = NULL, 16 the result is NULL, 32 x3d = NULL
#include "../mc_slam_amd/csrc/vba_host_triangulate.h"

#include "host_check.h"

using namespace vba_host;

static void tri_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_triangulate_problem> P(ok ? n : 0);
    std::vector<vba_triangulate_result> R(P.size());
    std::vector<vba_triangulate_problem*> pp(P.size());
    std::vector<vba_triangulate_result*> rr(P.size());
    std::vector<size_t> len(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[7];
        double c[41];
        ok = fread(hd, 4, 7, f) == 7 && fread(c, 8, 41, f) == 41 && hd[1] >= 0 && hd[3] >= 0 && hd[5] >= 0;
        if (!ok) break;
        vba_triangulate_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        len[k] = hd[1];
        p.n_matches = hd[0]; p.n_levels1 = hd[2]; p.n_levels2 = hd[4];
        std::memcpy(p.Rcw1, c, 72); std::memcpy(p.tcw1, c + 9, 24); std::memcpy(p.Ow1, c + 12, 24); std::memcpy(p.K1, c + 15, 32);
        std::memcpy(p.Rcw2, c + 19, 72); std::memcpy(p.tcw2, c + 28, 24); std::memcpy(p.Ow2, c + 31, 24); std::memcpy(p.K2, c + 34, 32);
        p.ratio_factor = c[38]; p.cos_max = c[39]; p.chi2_th = c[40];
        p.level_sigma2_1 = H.read<double>(f, hd[3], ok); p.scale_1 = H.read<double>(f, hd[3], ok);
        p.level_sigma2_2 = H.read<double>(f, hd[5], ok); p.scale_2 = H.read<double>(f, hd[5], ok);
        p.uv1 = H.read<double>(f, 2 * len[k], ok); p.uv2 = H.read<double>(f, 2 * len[k], ok);
        p.oct1 = H.read<uint8_t>(f, len[k], ok); p.oct2 = H.read<uint8_t>(f, len[k], ok);
        R[k].x3d = H.get<double>(3 * len[k]);
        R[k].reason = H.get<uint8_t>(len[k]);
        R[k].status = -7; R[k].n_accepted = -7;
        if (hd[6] & 1) p.uv2 = nullptr;
        if (hd[6] & 2) R[k].reason = nullptr;
        if (hd[6] & 8) p.scale_2 = nullptr;
        if (hd[6] & 32) R[k].x3d = nullptr;
        pp[k] = (hd[6] & 4) ? nullptr : &p;
        rr[k] = (hd[6] & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    TriCall C;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const TriBatch& B, void* hin) {
        printf("ok n_tot %zu l_tot %zu n_blocks %zu upload %zu back %zu total %zu desc %zu blk %zu lev %zu uv %zu oct %zu x3d %zu reason %zu", C.n_tot, C.l_tot,
               C.grid(), C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.A.desc, C.A.blk, C.A.lev, C.A.uv, C.A.oct, C.A.x3d, C.A.reason);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, blk); PRINT_BIND(B, hin, lev); PRINT_BIND(B, hin, uv); PRINT_BIND(B, hin, oct); PRINT_BIND(B, hin, x3d);
        PRINT_BIND(B, hin, reason);
        printf(" sum_desc %llu sum_blk %llu sum_lev %llu sum_uv %llu sum_oct %llu", checksum(at<char>(hin, C.A.desc), sizeof(TriDesc) * n),
               checksum(at<char>(hin, C.A.blk), sizeof(TriBlock) * C.n_blocks), checksum(at<char>(hin, C.A.lev), 8 * C.l_tot), checksum(at<char>(hin, C.A.uv), 32 * C.n_tot),
               checksum(at<char>(hin, C.A.oct), 2 * C.n_tot));
    }, [&](void* hout) {
        // what came back: double j of the x3d region is j, match i of the call has reason i mod 9
        double* x3d = at<double>(hout, C.A.L.in_back(C.A.x3d));
        unsigned char* reason = at<unsigned char>(hout, C.A.L.in_back(C.A.reason));
        for (size_t j = 0; j < 3 * C.n_tot; j++) x3d[j] = (double)j;
        for (size_t i = 0; i < C.n_tot; i++) reason[i] = (unsigned char)(i % 9);
    });
    if (!ran) return;
    long long s_acc = 0, s_status = 0, s_reason = 0;
    double s_x = 0;
    for (int k = 0; k < n; k++) {
        s_acc += R[k].n_accepted * (long long)(k + 1);
        s_status += R[k].status;
        for (size_t i = 0; i < len[k] && (size_t)P[k].n_matches == len[k]; i++) { s_reason += R[k].reason[i]; s_x += R[k].x3d[3 * i] + R[k].x3d[3 * i + 1] + R[k].x3d[3 * i + 2]; }
    }
    printf(" got_acc %lld got_status %lld got_reason %lld got_x %.0f\n", s_acc, s_status, s_reason, s_x);
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, tri_file); }
