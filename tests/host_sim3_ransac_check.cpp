// Sanitizer harness of the host half of vba_sim3_ransac (mc_slam_amd/csrc/vba_host_sim3_ransac.h, vba_host_arena.h): plain C++,
// built by tests/test_host_sim3_ransac.py with g++ -fsanitize=address,undefined.
//   host_sim3_ransac_check <file>...     one line per file: "ok key value ..." or "error <message>"
// RansacCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of
// its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per problem i32 n_pairs len n_hyp hlen fix_scale min_inliers best_inliers
// nulls want_counts, f64 K1[4] K2[4] best_S12[8], f64 p1c[len][3] p2c[len][3] max_err1[len] max_err2[len], i32 sample[hlen][3].
// n_pairs / n_hyp are the fields, len / hlen the arrays; nulls: 1 max_err2 = NULL, 2 inlier = NULL, 4 the problem itself is NULL,
// 8 sample = NULL, 16 the result is NULL
#include "../mc_slam_amd/csrc/vba_host_sim3_ransac.h"

#include "host_check.h"

using namespace vba_host;

static void ransac_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_sim3_ransac_problem> P(ok ? n : 0);
    std::vector<vba_sim3_ransac_result> R(P.size());
    std::vector<vba_sim3_ransac_problem*> pp(P.size());
    std::vector<vba_sim3_ransac_result*> rr(P.size());
    std::vector<size_t> len(P.size()), hlen(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[9];
        double sc[16];
        ok = fread(hd, 4, 9, f) == 9 && fread(sc, 8, 16, f) == 16 && hd[1] >= 0 && hd[3] >= 0;
        if (!ok) break;
        vba_sim3_ransac_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        len[k] = hd[1]; hlen[k] = hd[3];
        p.n_pairs = hd[0]; p.n_hyp = hd[2]; p.fix_scale = hd[4]; p.min_inliers = hd[5]; p.best_inliers = hd[6];
        std::memcpy(p.K1, sc, 32); std::memcpy(p.K2, sc + 4, 32); std::memcpy(p.best_S12, sc + 8, 64);
        p.p1c = H.read<double>(f, 3 * len[k], ok); p.p2c = H.read<double>(f, 3 * len[k], ok);
        p.max_err1 = H.read<double>(f, len[k], ok); p.max_err2 = H.read<double>(f, len[k], ok);
        p.sample = H.read<int32_t>(f, 3 * hlen[k], ok);
        R[k].inlier = H.get<uint8_t>(len[k]);
        std::memset(R[k].inlier, 7, len[k]);
        for (int q = 0; q < 8; q++) R[k].S12[q] = -1.0;
        if (hd[8]) R[k].hyp_inliers = H.get<int32_t>(hlen[k]);
        if (hd[7] & 1) p.max_err2 = nullptr;
        if (hd[7] & 2) R[k].inlier = nullptr;
        if (hd[7] & 8) p.sample = nullptr;
        pp[k] = (hd[7] & 4) ? nullptr : &p;
        rr[k] = (hd[7] & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    RansacCall C;
    const RansacOut* res = nullptr;
    std::vector<double> before(n);
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const RansacBatch& B, void* hin) {
        printf("ok n_tot %zu h_tot %zu want %d upload %zu back %zu total %zu download %zu desc %zu p %zu gate %zu sample %zu out %zu flag %zu cnt %zu hyp %zu", C.n_tot,
               C.h_tot, (int)C.want_counts, C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.download_bytes(), C.A.desc, C.A.p, C.A.gate, C.A.sample, C.A.out, C.A.flag,
               C.A.cnt, C.A.hyp);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, out); PRINT_BIND(B, hin, p); PRINT_BIND(B, hin, gate); PRINT_BIND(B, hin, sample); PRINT_BIND(B, hin, hyp);
        PRINT_BIND(B, hin, cnt); PRINT_BIND(B, hin, flag);
        printf(" sum_desc %llu sum_p %llu sum_gate %llu sum_sample %llu", checksum(at<char>(hin, C.A.desc), sizeof(RansacDesc) * n), checksum(at<char>(hin, C.A.p), 48 * C.n_tot),
               checksum(at<char>(hin, C.A.gate), 16 * C.n_tot), checksum(at<char>(hin, C.A.sample), 12 * C.h_tot));
    }, [&](void* hout) {
        // what came back: problem k has a hit (hypothesis 0) when k is even and it has hypotheses, best_hyp = n_hyp - 1 when k % 3 == 0;
        // pair i is flagged when i is odd, hypothesis j counted j
        RansacOut* r = at<RansacOut>(hout, C.A.L.in_back(C.A.out));
        unsigned char* flag = at<unsigned char>(hout, C.A.L.in_back(C.A.flag));
        int32_t* cnt = at<int32_t>(hout, C.A.L.in_back(C.A.cnt));   // read by unpack only when a caller wants the counts
        for (int k = 0; k < n; k++) {
            std::memset(&r[k], 0, sizeof r[k]);
            const bool hyp = P[k].n_hyp > 0;
            r[k].hit = (hyp && k % 2 == 0) ? 0 : -1;
            r[k].best_hyp = (hyp && k % 3 == 0) ? P[k].n_hyp - 1 : -1;
            r[k].its_done = k; r[k].n_inliers = 2 * k; r[k].best_inliers = 3 * k + 1;
            for (int q = 0; q < 8; q++) { r[k].S[q] = k + q; r[k].best_S[q] = 100 + k + q; }
            before[k] = P[k].best_S12[0];
        }
        for (size_t i = 0; i < C.n_tot; i++) flag[i] = i & 1;
        for (size_t i = 0; i < C.h_tot && C.want_counts; i++) cnt[i] = (int32_t)i;
        res = r;
    });
    if (!ran) return;
    unsigned long long s_its = 0, s_best = 0, s_flag = 0, s_cnt = 0, s_keep = 0;
    double s_S = 0, s_bS = 0;
    for (int k = 0; k < n; k++) {
        s_its += R[k].its_done; s_best += P[k].best_inliers; s_S += R[k].S12[7]; s_bS += P[k].best_S12[7];
        if (res[k].best_hyp < 0 && P[k].best_S12[0] == before[k]) s_keep++;
        for (size_t i = 0; i < len[k] && (size_t)P[k].n_pairs == len[k]; i++) s_flag += R[k].inlier[i];
        for (size_t j = 0; j < hlen[k] && R[k].hyp_inliers; j++) s_cnt += R[k].hyp_inliers[j];
    }
    printf(" got_its %llu got_best %llu got_S7 %.0f got_bestS7 %.0f got_flag %llu got_cnt %llu got_keep %llu\n", s_its, s_best, s_S, s_bS, s_flag, s_cnt, s_keep);
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, ransac_file); }
