// Sanitizer harness of the host halves of vba_sim3_optimize and vba_pose_optimize (mc_slam_amd/csrc/vba_host_sim3.h,
// vba_host_pose.h, vba_host_arena.h): plain C++, built by tests/test_host_small.py with g++ -fsanitize=address,undefined.
//   host_small_check sim3 <file>...     one line per file: "ok key value ..." or "error <message>"
//   host_small_check pose <file>...     the same
//   host_small_check inverse <file>...  "ok <n*n values>" or "singular"
// Sim3Call and PoseCall run as the library's driver runs them (run_call, tests/host_check.h); every array of the callers is a heap
// block of its exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into
// the arena.
// Files (little-endian, written by the test):
//   sim3: i32 n, then per problem i32 n_pairs len fix_scale its1 its2_bad its2_clean min_inliers nulls want_chi2, f64 S12[8] K1[4]
//         K2[4] th2 huber, f64 p1c[len][3] p2c[len][3] uv1[len][2] uv2[len][2] w1[len] w2[len].  n_pairs is the field, len the arrays;
//         nulls: 1 uv2 = NULL, 2 outlier = NULL, 4 the problem itself is NULL
//   pose: i32 n, then per frame i32 kind compute_marg n_obs n_obs_last len len_last nulls, f64 nav[22] nav_last[22] K[4] T_cb[7]
//         g_w[3] imu_meas[61] imu_cov_pvphi[81] prior_nav[22] prior_info[225] inv_bg inv_ba, f64 obs_pw[len][3] obs_uv[len][2] obs_w[len]
//         last_pw[len_last][3] last_uv[len_last][2] last_w[len_last].  nulls: 1 obs_uv = NULL, 2 last_uv = NULL, 4 outlier = NULL,
//         8 the frame itself is NULL
//   inverse: i32 n, f64 A[n][n]
#include "../mc_slam_amd/csrc/vba_host_pose.h"
#include "../mc_slam_amd/csrc/vba_host_sim3.h"

#include "host_check.h"

using namespace vba_host;

static void sim3_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_sim3_problem> P(ok ? n : 0);
    std::vector<vba_sim3_result> R(P.size());
    std::vector<vba_sim3_problem*> pp(P.size());
    std::vector<vba_sim3_result*> rr(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[9];
        double sc[18];
        ok = fread(hd, 4, 9, f) == 9 && fread(sc, 8, 18, f) == 18 && hd[1] >= 0;
        if (!ok) break;
        vba_sim3_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        const size_t len = hd[1];
        p.n_pairs = hd[0]; p.fix_scale = hd[2]; p.its_stage1 = hd[3]; p.its_stage2_bad = hd[4]; p.its_stage2_clean = hd[5]; p.min_inliers = hd[6];
        std::memcpy(p.S12, sc, 64); std::memcpy(p.K1, sc + 8, 32); std::memcpy(p.K2, sc + 12, 32);
        p.th2 = sc[16]; p.huber = sc[17];
        p.p1c = H.read<double>(f, 3 * len, ok); p.p2c = H.read<double>(f, 3 * len, ok);
        p.uv1 = H.read<double>(f, 2 * len, ok); p.uv2 = H.read<double>(f, 2 * len, ok);
        p.w1 = H.read<double>(f, len, ok); p.w2 = H.read<double>(f, len, ok);
        R[k].outlier = H.get<uint8_t>(len);
        if (hd[8]) { R[k].chi2_12 = H.get<double>(len); R[k].chi2_21 = H.get<double>(len); }
        if (hd[7] & 1) p.uv2 = nullptr;
        if (hd[7] & 2) R[k].outlier = nullptr;
        pp[k] = (hd[7] & 4) ? nullptr : &p;
        rr[k] = &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    Sim3Call C;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const Sim3Batch& B, void* hin) {
        printf("ok n_tot %zu want_chi2 %d upload %zu back %zu total %zu download %zu desc %zu p %zu uv %zu w %zu out %zu flag %zu c %zu", C.n_tot, (int)C.want_chi2,
               C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.download_bytes(), C.A.desc, C.A.p, C.A.uv, C.A.w, C.A.out, C.A.flag, C.A.c);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, out); PRINT_BIND(B, hin, p); PRINT_BIND(B, hin, uv); PRINT_BIND(B, hin, w); PRINT_BIND(B, hin, c);
        PRINT_BIND(B, hin, flag);
        printf(" sum_desc %llu sum_p %llu sum_uv %llu sum_w %llu", checksum(at<char>(hin, C.A.desc), sizeof(Sim3Desc) * n), checksum(at<char>(hin, C.A.p), 48 * C.n_tot),
               checksum(at<char>(hin, C.A.uv), 32 * C.n_tot), checksum(at<char>(hin, C.A.w), 16 * C.n_tot));
    }, [&](void* hout) {
        // what came back: out record k says k, pair i is flagged when i is odd, its chi2 are 2 i and 2 i + 1
        Sim3Out* res = at<Sim3Out>(hout, C.A.L.in_back(C.A.out));
        unsigned char* flag = at<unsigned char>(hout, C.A.L.in_back(C.A.flag));
        double* cc = at<double>(hout, C.A.L.in_back(C.A.c));
        for (int k = 0; k < n; k++) { std::memset(&res[k], 0, sizeof res[k]); res[k].n_inliers = k; for (int q = 0; q < 8; q++) res[k].S[q] = k + q; }
        for (size_t i = 0; i < C.n_tot; i++) flag[i] = i & 1;
        for (size_t i = 0; i < 2 * C.n_tot && C.want_chi2; i++) cc[i] = (double)i;
    });
    if (!ran) return;
    unsigned long long s_in = 0, s_flag = 0;
    double s_12 = 0, s_21 = 0, s_S = 0;
    for (int k = 0; k < n; k++) {
        s_in += R[k].n_inliers; s_S += P[k].S12[7];
        for (int i = 0; i < P[k].n_pairs; i++) {
            s_flag += R[k].outlier[i];
            if (R[k].chi2_12) { s_12 += R[k].chi2_12[i]; s_21 += R[k].chi2_21[i]; }
        }
    }
    printf(" got_inliers %llu got_S7 %.0f got_flag %llu got_chi12 %.0f got_chi21 %.0f\n", s_in, s_S, s_flag, s_12, s_21);
}

static void pose_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_frame_problem> P(ok ? n : 0);
    std::vector<vba_frame_result> R(P.size());
    std::vector<vba_frame_problem*> pp(P.size());
    std::vector<vba_frame_result*> rr(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[7];
        ok = fread(hd, 4, 7, f) == 7 && hd[4] >= 0 && hd[5] >= 0;
        if (!ok) break;
        vba_frame_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        p.last_is_frame = hd[0]; p.compute_marg = hd[1]; p.n_obs = hd[2]; p.n_obs_last = hd[3];
        const size_t len = hd[4], len_last = hd[5];
        ok = fread(p.nav, 8, 22, f) == 22 && fread(p.nav_last, 8, 22, f) == 22 && fread(p.K, 8, 4, f) == 4 && fread(p.T_cb, 8, 7, f) == 7 &&
             fread(p.g_w, 8, 3, f) == 3 && fread(p.imu_meas, 8, 61, f) == 61 && fread(p.imu_cov_pvphi, 8, 81, f) == 81 &&
             fread(p.prior_nav, 8, 22, f) == 22 && fread(p.prior_info, 8, 225, f) == 225 && fread(&p.inv_bg_rw2, 8, 1, f) == 1 &&
             fread(&p.inv_ba_rw2, 8, 1, f) == 1;
        p.obs_pw = H.read<double>(f, 3 * len, ok); p.obs_uv = H.read<double>(f, 2 * len, ok); p.obs_w = H.read<double>(f, len, ok);
        p.last_pw = H.read<double>(f, 3 * len_last, ok); p.last_uv = H.read<double>(f, 2 * len_last, ok); p.last_w = H.read<double>(f, len_last, ok);
        R[k].outlier = H.get<uint8_t>(len);
        R[k].outlier_last = H.get<uint8_t>(len_last);
        if (hd[6] & 1) p.obs_uv = nullptr;
        if (hd[6] & 2) p.last_uv = nullptr;
        if (hd[6] & 4) R[k].outlier = nullptr;
        pp[k] = (hd[6] & 8) ? nullptr : &p;
        rr[k] = &R[k];
    }
    if (!ok) { printf("error load\n"); return; }
    PoseCall C;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const PoseBatch& B, void* hin) {
        const FrameDesc* desc = at<FrameDesc>(hin, C.A.desc);
        printf("ok n_tot %zu upload %zu back %zu total %zu desc %zu pw %zu uv %zu w %zu out %zu lvl %zu err %zu n_frames %d", C.n_tot, C.A.L.upload_bytes(), C.A.L.back_bytes(),
               C.A.L.total_bytes(), C.A.desc, C.A.pw, C.A.uv, C.A.w, C.A.out, C.A.lvl, C.A.err, B.n_frames);
        PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, out); PRINT_BIND(B, hin, pw); PRINT_BIND(B, hin, uv); PRINT_BIND(B, hin, w); PRINT_BIND(B, hin, err);
        PRINT_BIND(B, hin, lvl);
        printf(" sum_pw %llu sum_uv %llu sum_w %llu", checksum(at<char>(hin, C.A.pw), 24 * C.n_tot), checksum(at<char>(hin, C.A.uv), 16 * C.n_tot),
               checksum(at<char>(hin, C.A.w), 8 * C.n_tot));
        // the descriptors: the integers, and a checksum over the fields a frame's values are copied into
        unsigned long long s_int = 0, s_val = 0;
        double info_err = 0;
        for (int k = 0; k < n; k++) {
            const FrameDesc& d = desc[k];
            const int iv[8] = {d.last_is_frame, d.compute_marg, d.n_obs, d.n_last, d.obs0, d.last0, d.pad0, d.pad1};
            for (int q = 0; q < 8; q++) s_int += (unsigned long long)(8 * k + q + 1) * (unsigned)iv[q];
            std::vector<double> v;
            auto add = [&v](const double* p, size_t m) { v.insert(v.end(), p, p + m); };
            add(d.nav, 22); add(d.nav_last, 22); add(d.prior_nav, 22); add(d.K, 4); add(d.tcb, 3); add(d.g, 3); add(d.meas, 61); add(d.prior_info, 225);
            add(&d.inv_bg, 1); add(&d.inv_ba, 1); add(&d.hub_prior, 1); add(&d.hub_pvr, 1); add(&d.hub_bias, 1); add(&d.hub_mono, 1);
            s_val += (unsigned long long)(k + 1) * checksum(v.data(), 8 * v.size());
            for (int i = 0; i < 9 && d.last_is_frame != VBA_FRAME_VISION; i++)     // info_pvr * cov = I, to rounding
                for (int j = 0; j < 9; j++) {
                    double s = 0;
                    for (int q = 0; q < 9; q++) s += d.info_pvr[9 * i + q] * P[k].imu_cov_pvphi[9 * q + j];
                    info_err = std::max(info_err, std::fabs(s - (i == j)));
                }
        }
        printf(" sum_int %llu sum_val %llu info_err %.3g", s_int, s_val, info_err);
    }, [&](void* hout) {
        // what came back: out record k says k, observation i is an outlier when i is odd
        FrameOut* res = at<FrameOut>(hout, C.A.L.in_back(C.A.out));
        unsigned char* lvl = at<unsigned char>(hout, C.A.L.in_back(C.A.lvl));
        for (int k = 0; k < n; k++) { std::memset(&res[k], 0, sizeof res[k]); res[k].n_inliers = k; for (int q = 0; q < 22; q++) res[k].nav[q] = k + q; }
        for (size_t i = 0; i < C.n_tot; i++) lvl[i] = i & 1;
    });
    if (!ran) return;
    unsigned long long s_in = 0, s_out = 0, s_last = 0;
    double s_nav = 0;
    for (int k = 0; k < n; k++) {
        const int n_last = P[k].last_is_frame == VBA_FRAME_FRAME ? P[k].n_obs_last : 0;
        s_in += R[k].n_inliers; s_nav += P[k].nav[21];
        for (int i = 0; i < P[k].n_obs; i++) s_out += R[k].outlier[i];
        for (int i = 0; i < n_last; i++) s_last += R[k].outlier_last[i];
    }
    printf(" got_inliers %llu got_nav21 %.0f got_outlier %llu got_outlier_last %llu\n", s_in, s_nav, s_out, s_last);
}

static void inverse_file(FILE* f) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 1 || n > 15) { printf("error load\n"); return; }
    std::vector<double> A((size_t)n * n), Ai((size_t)n * n);
    if (fread(A.data(), 8, A.size(), f) != A.size()) { printf("error load\n"); return; }
    if (!inverse_host(n, A.data(), Ai.data())) { printf("singular\n"); return; }
    printf("ok");
    for (double v : Ai) printf(" %.17g", v);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "sim3") return for_each_file(argc, argv, 2, sim3_file);
    if (mode == "pose") return for_each_file(argc, argv, 2, pose_file);
    if (mode == "inverse") return for_each_file(argc, argv, 2, inverse_file);
    return 2;
}
