// Sanitizer harness of the host half of vba_two_view_init (mc_slam_amd/csrc/vba_host_two_view.h, vba_host_arena.h): plain C++,
// built by tests/test_host_two_view.py with g++ -fsanitize=address,undefined.
//   host_two_view_check <file>...     one line per file: "ok key value ..." or "error <message>"
// TwoViewCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of
// its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per pair i32 n_keys1 len1 n_keys2 len2 n_matches lenm n_hyp lenh nulls
// min_triangulated, f64 K[4] sigma min_parallax, f64 uv1[len1][2] uv2[len2][2], i32 match[lenm][2] sets[lenh][8].  n_* are the
// fields, len* the arrays; nulls: 1 uv2, 2 inlier_f, 4 the problem itself, 8 sets, 16 the result, 32 x3d, 64 match, 128 both
// hyp_score arrays (legal), 256 triangulated, 512 uv1, 1024 inlier_h = NULL
#include "../mc_slam_amd/csrc/vba_host_two_view.h"

#include "host_check.h"

using namespace vba_host;

static void tv_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_two_view_problem> P(ok ? n : 0);
    std::vector<vba_two_view_result> R(P.size());
    std::vector<vba_two_view_problem*> pp(P.size());
    std::vector<vba_two_view_result*> rr(P.size());
    std::vector<size_t> l1(P.size()), lm(P.size()), lh(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[10];
        double c[6];
        ok = fread(hd, 4, 10, f) == 10 && fread(c, 8, 6, f) == 6 && hd[1] >= 0 && hd[3] >= 0 && hd[5] >= 0 && hd[7] >= 0;
        if (!ok) break;
        vba_two_view_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        l1[k] = hd[1]; lm[k] = hd[5]; lh[k] = hd[7];
        p.n_keys1 = hd[0]; p.n_keys2 = hd[2]; p.n_matches = hd[4]; p.n_hyp = hd[6]; p.min_triangulated = hd[9];
        std::memcpy(p.K, c, 32);
        p.sigma = c[4]; p.min_parallax = c[5];
        p.uv1 = H.read<double>(f, 2 * (size_t)hd[1], ok); p.uv2 = H.read<double>(f, 2 * (size_t)hd[3], ok);
        p.match = H.read<int32_t>(f, 2 * lm[k], ok); p.sets = H.read<int32_t>(f, 8 * lh[k], ok);
        R[k].inlier_h = H.fill<uint8_t>(lm[k], 7); R[k].inlier_f = H.fill<uint8_t>(lm[k], 7);
        R[k].x3d = H.fill<double>(3 * l1[k], 7.0); R[k].triangulated = H.fill<uint8_t>(l1[k], 7);
        R[k].hyp_score_h = H.fill<double>(lh[k], 7.0); R[k].hyp_score_f = H.fill<double>(lh[k], 7.0);
        R[k].status = -7; R[k].ok = -7;
        for (int i = 0; i < 9; i++) R[k].R21[i] = 7.0;
        const int nulls = hd[8];
        if (nulls & 1) p.uv2 = nullptr;
        if (nulls & 2) R[k].inlier_f = nullptr;
        if (nulls & 8) p.sets = nullptr;
        if (nulls & 32) R[k].x3d = nullptr;
        if (nulls & 64) p.match = nullptr;
        if (nulls & 128) R[k].hyp_score_h = R[k].hyp_score_f = nullptr;
        if (nulls & 256) R[k].triangulated = nullptr;
        if (nulls & 512) p.uv1 = nullptr;
        if (nulls & 1024) R[k].inlier_h = nullptr;
        pp[k] = (nulls & 4) ? nullptr : &p;
        rr[k] = (nulls & 16) ? nullptr : &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    TwoViewCall C;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const TvBatch& B, void* hin) {
        printf("ok k1 %zu k2 %zu m %zu h %zu want %d upload %zu back %zu down %zu total %zu", C.T.k1, C.T.k2, C.T.m, C.T.h, (int)C.T.want_scores, C.A.L.upload_bytes(),
               C.A.L.back_bytes(), C.download_bytes(), C.A.L.total_bytes());
        printf(" desc %zu uv1 %zu uv2 %zu match %zu sets %zu out %zu flag_h %zu flag_f %zu tri %zu x3d %zu score_h %zu score_f %zu hyp_h %zu hyp_f %zu rt_state %zu rt_cos %zu rt_x %zu",
               C.A.desc, C.A.uv1, C.A.uv2, C.A.match, C.A.sets, C.A.out, C.A.flag_h, C.A.flag_f, C.A.tri, C.A.x3d, C.A.score_h, C.A.score_f, C.A.hyp_h, C.A.hyp_f, C.A.rt_state, C.A.rt_cos, C.A.rt_x);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, uv1); PRINT_BIND(B, hin, uv2); PRINT_BIND(B, hin, match); PRINT_BIND(B, hin, sets); PRINT_BIND(B, hin, out);
        PRINT_BIND(B, hin, flag_h); PRINT_BIND(B, hin, flag_f); PRINT_BIND(B, hin, tri); PRINT_BIND(B, hin, x3d); PRINT_BIND(B, hin, score_h);
        PRINT_BIND(B, hin, score_f); PRINT_BIND(B, hin, hyp_h); PRINT_BIND(B, hin, hyp_f); PRINT_BIND(B, hin, rt_state); PRINT_BIND(B, hin, rt_cos);
        PRINT_BIND(B, hin, rt_x);
        printf(" sum_desc %llu sum_uv1 %llu sum_uv2 %llu sum_match %llu sum_sets %llu", checksum(at<char>(hin, C.A.desc), sizeof(TvDesc) * n),
               checksum(at<char>(hin, C.A.uv1), 16 * C.T.k1), checksum(at<char>(hin, C.A.uv2), 16 * C.T.k2), checksum(at<char>(hin, C.A.match), 8 * C.T.m),
               checksum(at<char>(hin, C.A.sets), 32 * C.T.h));
    }, [&](void* hout) {
        // what came back: pair k is ok when k is odd; flag_h[i] = i % 2, flag_f[i] = (i % 3 == 0), tri[j] = j % 2, double j of x3d is j,
        // score_h[h] = h, score_f[h] = 2 h (i, j, h count through the call)
        TvOut* res = at<TvOut>(hout, C.A.L.in_back(C.A.out));
        unsigned char* fh = at<unsigned char>(hout, C.A.L.in_back(C.A.flag_h));
        unsigned char* ff = at<unsigned char>(hout, C.A.L.in_back(C.A.flag_f));
        unsigned char* tri = at<unsigned char>(hout, C.A.L.in_back(C.A.tri));
        double* x3d = at<double>(hout, C.A.L.in_back(C.A.x3d));
        double* sh = at<double>(hout, C.A.L.in_back(C.A.score_h));   // beyond the downloaded bytes without score arrays: never touched then
        double* sf = at<double>(hout, C.A.L.in_back(C.A.score_f));
        for (int k = 0; k < n; k++) {
            std::memset(&res[k], 0, sizeof(TvOut));
            res[k].ok = k % 2; res[k].model = 1 + k % 2; res[k].reason = k % 6; res[k].best_hyp_h = k; res[k].best_hyp_f = -1; res[k].n_rt = 4; res[k].best_rt = 3;
            res[k].n_inliers_h = 2 * k; res[k].n_inliers_f = 3 * k;
            for (int i = 0; i < 8; i++) { res[k].rt_good[i] = k + i; res[k].rt_parallax[i] = 0.5 * i; }
            res[k].score_h = 1.5; res[k].score_f = 2.5; res[k].rh = 0.375;
            for (int i = 0; i < 9; i++) { res[k].H21[i] = i; res[k].F21[i] = -i; res[k].R21[i] = 10 + i; }
            for (int i = 0; i < 3; i++) res[k].t21[i] = 20 + i;
        }
        for (size_t i = 0; i < C.T.m; i++) { fh[i] = (unsigned char)(i % 2); ff[i] = (unsigned char)(i % 3 == 0); }
        for (size_t j = 0; j < C.T.k1; j++) tri[j] = (unsigned char)(j % 2);
        for (size_t j = 0; j < 3 * C.T.k1; j++) x3d[j] = (double)j;
        if (C.T.want_scores) for (size_t h = 0; h < C.T.h; h++) { sh[h] = (double)h; sf[h] = 2.0 * h; }
    });
    if (!ran) return;
    long long s_ok = 0, s_head = 0, s_fh = 0, s_ff = 0, s_tri = 0;
    double s_x = 0, s_R = 0, s_sc = 0, s_mat = 0;
    for (int k = 0; k < n; k++) {
        const vba_two_view_result& r = R[k];
        s_ok += r.ok;
        s_head += r.status + r.model + r.reason + r.best_hyp_h + r.best_hyp_f + r.n_inliers_h + r.n_inliers_f + r.n_rt + r.best_rt + r.rt_good[7];
        s_mat += r.H21[8] + r.F21[8] + r.rt_parallax[7] + r.score_h + r.score_f + r.rh;
        if ((size_t)P[k].n_matches == lm[k]) for (size_t i = 0; i < lm[k]; i++) { s_fh += r.inlier_h[i]; s_ff += r.inlier_f[i]; }
        if ((size_t)P[k].n_keys1 == l1[k]) for (size_t j = 0; j < l1[k]; j++) { s_tri += r.triangulated[j]; s_x += r.x3d[3 * j] + r.x3d[3 * j + 1] + r.x3d[3 * j + 2]; }
        s_R += r.R21[0] + r.R21[8] + r.t21[2];
        if (r.hyp_score_h && (size_t)P[k].n_hyp == lh[k]) for (size_t h = 0; h < lh[k]; h++) s_sc += r.hyp_score_h[h] + r.hyp_score_f[h];
    }
    printf(" got_ok %lld got_head %lld got_fh %lld got_ff %lld got_tri %lld got_x %.0f got_R %.0f got_sc %.0f got_mat %.3f\n", s_ok, s_head, s_fh, s_ff, s_tri, s_x,
           s_R, s_sc, s_mat);
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, tv_file); }
