// Sanitizer harness of the host half of vba_mappoint_update (mc_slam_amd/csrc/vba_host_mappoint.h, vba_host_arena.h): plain C++,
// built by tests/test_host_mappoint.py with g++ -fsanitize=address,undefined.
//   host_mappoint_check <file>...     one line per file: "ok key value ..." or "error <message>"
// MapPointCall runs as the library's driver runs it (run_call, tests/host_check.h); every array of the callers is a heap block of its
// exact size, so any overrun is an ASan report.  bind_<field>: where the kernel's argument points, as an offset into the arena.
// Files (little-endian, written by the test): i32 n, then per problem i32 hd[6] = n_kf len_kf n_pt len_pt len_obs nulls, f64
// kf_center[len_kf][3], u8 kf_bad[len_kf], u8 what[len_pt], f64 pos[len_pt][3], i32 ref_kf[len_pt], f64 ref_scale[len_pt]
// ref_top_scale[len_pt], i32 obs_begin[len_pt + 1] obs_kf[len_obs], u8 obs_desc[len_obs][32].  n_kf / n_pt are the fields, len_kf /
// len_pt the arrays.  nulls: 1 the problem, 2 the result, 4 kf_center, 8 kf_bad, 16 what, 32 pos, 64 ref_kf, 128 ref_scale,
// 256 ref_top_scale, 512 obs_begin, 1024 obs_kf, 2048 obs_desc, 4096 the result's best_obs, 8192 its normal_state, 16384 its desc
#include "../mc_slam_amd/csrc/vba_host_mappoint.h"

#include "host_check.h"

using namespace vba_host;

static void mappoint_file(FILE* f) {
    Heap H;
    int32_t n = 0;
    bool ok = fread(&n, 4, 1, f) == 1 && n >= 0;
    std::vector<vba_mappoint_problem> P(ok ? n : 0);
    std::vector<vba_mappoint_result> R(P.size());
    std::vector<vba_mappoint_problem*> pp(P.size());
    std::vector<vba_mappoint_result*> rr(P.size());
    std::vector<size_t> len(P.size());
    for (size_t k = 0; k < P.size() && ok; k++) {
        int32_t hd[6];
        ok = fread(hd, 4, 6, f) == 6 && hd[1] >= 0 && hd[3] >= 0 && hd[4] >= 0;
        if (!ok) break;
        vba_mappoint_problem& p = P[k];
        std::memset(&p, 0, sizeof p);
        std::memset(&R[k], 0, sizeof R[k]);
        const size_t lk = hd[1], lp = hd[3], lo = hd[4];
        len[k] = lp;
        p.n_kf = hd[0]; p.n_pt = hd[2];
        p.kf_center = H.read<double>(f, 3 * lk, ok); p.kf_bad = H.read<uint8_t>(f, lk, ok);
        p.what = H.read<uint8_t>(f, lp, ok); p.pos = H.read<double>(f, 3 * lp, ok); p.ref_kf = H.read<int32_t>(f, lp, ok);
        p.ref_scale = H.read<double>(f, lp, ok); p.ref_top_scale = H.read<double>(f, lp, ok);
        p.obs_begin = H.read<int32_t>(f, lp + 1, ok); p.obs_kf = H.read<int32_t>(f, lo, ok); p.obs_desc = H.read<uint8_t>(f, 32 * lo, ok);
        vba_mappoint_result& r = R[k];
        r.best_obs = H.fill<int32_t>(lp, -7); r.best_median = H.fill<int32_t>(lp, -7); r.n_desc = H.fill<int32_t>(lp, -7);
        r.desc = H.fill<uint8_t>(32 * lp, 77); r.normal = H.fill<double>(3 * lp, -7.0); r.dist_max = H.fill<double>(lp, -7.0);
        r.dist_min = H.fill<double>(lp, -7.0); r.desc_state = H.fill<uint8_t>(lp, 255); r.normal_state = H.fill<uint8_t>(lp, 255);
        r.status = -7; r.n_desc_done = -7; r.n_normal_done = -7;
        const int nl = hd[5];
        if (nl & 4) p.kf_center = nullptr;
        if (nl & 8) p.kf_bad = nullptr;
        if (nl & 16) p.what = nullptr;
        if (nl & 32) p.pos = nullptr;
        if (nl & 64) p.ref_kf = nullptr;
        if (nl & 128) p.ref_scale = nullptr;
        if (nl & 256) p.ref_top_scale = nullptr;
        if (nl & 512) p.obs_begin = nullptr;
        if (nl & 1024) p.obs_kf = nullptr;
        if (nl & 2048) p.obs_desc = nullptr;
        if (nl & 4096) r.best_obs = nullptr;
        if (nl & 8192) r.normal_state = nullptr;
        if (nl & 16384) r.desc = nullptr;
        pp[k] = (nl & 1) ? nullptr : &p;
        rr[k] = (nl & 2) ? nullptr : &r;
    }
    if (!ok) { printf("error load\n"); return; }
    MapPointCall C;
    void* staged = nullptr;
    const bool ran = run_call(H, C, n, pp.data(), rr.data(), [&](const MpBatch& B, void* hin) {
        staged = hin;
        printf("ok pts %zu kf %zu items %zu big %zu obs_tot %zu desc_tot %zu grid %zu upload %zu back %zu total %zu item %zu center %zu obs %zu desc %zu best %zu "
               "nrm %zu nstate %zu n_items %d n_big %d",
               C.T.pts, C.T.kf, C.T.items, C.T.big, C.T.obs, C.T.desc, C.grid(), C.A.L.upload_bytes(), C.A.L.back_bytes(), C.A.L.total_bytes(), C.A.item,
               C.A.center, C.A.obs, C.A.desc, C.A.best, C.A.nrm, C.A.nstate, B.n_items, B.n_big);
        PRINT_BIND(B, hin, item); PRINT_BIND(B, hin, center); PRINT_BIND(B, hin, obs); PRINT_BIND(B, hin, desc); PRINT_BIND(B, hin, best);
        PRINT_BIND(B, hin, nrm); PRINT_BIND(B, hin, nstate);
        printf(" sum_item %llu sum_center %llu sum_obs %llu sum_desc %llu", checksum(at<char>(hin, C.A.item), sizeof(MpItem) * C.T.items),
               checksum(at<char>(hin, C.A.center), 24 * C.T.kf), checksum(at<char>(hin, C.A.obs), 4 * C.T.obs), checksum(at<char>(hin, C.A.desc), 32 * C.T.desc));
    }, [&](void* hout) {
        // what came back: item k has the key ((7 k mod 257) << 16) | (3 k mod N) (-1 without a descriptor part), nrm[j] = k + j / 8 and
        // nstate 3 when k is a multiple of 5, else 0 (1 without a normal part)
        auto back = [&](size_t off) { return C.A.L.in_back(off); };
        int32_t* best = at<int32_t>(hout, back(C.A.best));
        double* nrm = at<double>(hout, back(C.A.nrm));
        unsigned char* ns = at<unsigned char>(hout, back(C.A.nstate));
        const MpItem* item = at<MpItem>(staged, C.A.item);
        for (size_t k = 0; k < C.T.items; k++) {
            best[k] = item[k].n_desc ? (int32_t)((((7 * k) % 257) << 16) | ((3 * k) % (size_t)item[k].n_desc)) : -1;
            for (int j = 0; j < 5; j++) nrm[5 * k + j] = (double)k + j / 8.0;
            ns[k] = (unsigned char)(item[k].n_obs ? (k % 5 == 0 ? 3 : 0) : 1);
        }
    });
    if (!ran) return;
    long long s_status = 0, s_ndd = 0, s_nnd = 0, s_bo = 0, s_bm = 0, s_nd = 0, s_de = 0, s_ds = 0, s_ns = 0;
    double s_no = 0, s_dx = 0, s_dn = 0;
    for (int k = 0; k < n; k++) {
        s_status += R[k].status; s_ndd += R[k].n_desc_done * (long long)(k + 1); s_nnd += R[k].n_normal_done * (long long)(k + 1);
        for (size_t i = 0; i < len[k] && (size_t)P[k].n_pt == len[k]; i++) {
            s_bo += R[k].best_obs[i] * (long long)(i % 13 + 1); s_bm += R[k].best_median[i] * (long long)(i % 11 + 1); s_nd += R[k].n_desc[i] * (long long)(i % 7 + 1);
            for (int b = 0; b < 32; b++) s_de += R[k].desc[32 * i + b] * (long long)((i + b) % 5 + 1);
            s_ds += R[k].desc_state[i] * (long long)(i % 5 + 1); s_ns += R[k].normal_state[i] * (long long)(i % 3 + 1);
            s_no += R[k].normal[3 * i] + 2 * R[k].normal[3 * i + 1] + 4 * R[k].normal[3 * i + 2]; s_dx += R[k].dist_max[i]; s_dn += R[k].dist_min[i];
        }
    }
    printf(" got_status %lld got_ndd %lld got_nnd %lld got_bo %lld got_bm %lld got_nd %lld got_de %lld got_ds %lld got_ns %lld got_no8 %lld got_dx8 %lld got_dn8 %lld\n",
           s_status, s_ndd, s_nnd, s_bo, s_bm, s_nd, s_de, s_ds, s_ns, (long long)(s_no * 8), (long long)(s_dx * 8), (long long)(s_dn * 8));
}

int main(int argc, char** argv) { return for_each_file(argc, argv, 1, mappoint_file); }
