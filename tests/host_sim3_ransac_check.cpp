// Sanitizer harness of the host half of vba_sim3_ransac (mc_slam_amd/csrc/vba_host_sim3_ransac.h, vba_host_arena.h): plain C++,
// built by tests/test_host_sim3_ransac.py with g++ -fsanitize=address,undefined.
//   host_sim3_ransac_check <file>...     one line per file: "ok key value ..." or "error <message>"
// check, describe and pack run as the driver runs them -- above 256 problems on several threads, as small_pack_threads does --
// into malloc'ed blocks of exactly upload_bytes(); unpack reads a block of exactly the downloaded bytes and writes result arrays of
// exactly the caller's sizes, so any overrun is an ASan report.  Every array of the callers is a heap block of its exact size, too.
// Checksums: sum of (2 i + 1) * word i over the 64-bit words of a region's payload, mod 2^64.
// Files (little-endian, written by the test): i32 n, then per problem i32 n_pairs len n_hyp hlen fix_scale min_inliers best_inliers
// nulls want_counts, f64 K1[4] K2[4] best_S12[8], f64 p1c[len][3] p2c[len][3] max_err1[len] max_err2[len], i32 sample[hlen][3].
// n_pairs / n_hyp are the fields, len / hlen the arrays; nulls: 1 max_err2 = NULL, 2 inlier = NULL, 4 the problem itself is NULL,
// 8 sample = NULL, 16 the result is NULL
#include "../mc_slam_amd/csrc/vba_host_sim3_ransac.h"

#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

using namespace vba_host;

struct Heap {   // exact-size heap blocks, freed at the end of a file
    std::vector<void*> all;
    template <class T> T* get(size_t n) { void* p = malloc(n * sizeof(T) + (n == 0)); all.push_back(p); return static_cast<T*>(p); }
    template <class T> T* read(FILE* f, size_t n, bool& ok) { T* p = get<T>(n); ok = ok && (n == 0 || fread(p, sizeof(T), n, f) == n); return p; }
    ~Heap() { for (void* p : all) free(p); }
};

static unsigned long long checksum(const void* p, size_t bytes) {
    unsigned long long s = 0, w;
    for (size_t i = 0; i < bytes / 8; i++) { std::memcpy(&w, static_cast<const char*>(p) + 8 * i, 8); s += (2 * i + 1) * w; }
    return s;
}

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
    size_t n_tot = 0, h_tot = 0;
    bool want = false;
    std::string err;
    if (check_sim3_ransac(n, pp.data(), rr.data(), n_tot, h_tot, want, err)) { printf("error %s\n", err.c_str()); return; }
    const RansacArena A(n, n_tot, h_tot);
    void* hin = H.get<char>(A.L.upload_bytes());
    RansacDesc* desc = at<RansacDesc>(hin, A.desc);
    describe_sim3_ransac(n, pp.data(), desc);
    auto pack = [&](int k) { pack_sim3_ransac(pp[k], desc[k], at<double>(hin, A.p), at<double>(hin, A.gate), at<int32_t>(hin, A.sample)); };
    if (n >= 256) {   // the threaded path: problem k goes to thread k mod 4
        std::vector<std::thread> th;
        for (int t = 0; t < 4; t++) th.emplace_back([&, t] { for (int k = t; k < n; k += 4) pack(k); });
        for (auto& t : th) t.join();
    } else
        for (int k = 0; k < n; k++) pack(k);
    printf("ok n_tot %zu h_tot %zu want %d upload %zu back %zu total %zu download %zu desc %zu p %zu gate %zu sample %zu out %zu flag %zu cnt %zu hyp %zu", n_tot,
           h_tot, (int)want, A.L.upload_bytes(), A.L.back_bytes(), A.L.total_bytes(), A.download_bytes(want), A.desc, A.p, A.gate, A.sample, A.out, A.flag,
           A.cnt, A.hyp);
    std::vector<int32_t> smp(3 * h_tot + (h_tot & 1 ? 1 : 0), 0);   // the triples, padded to whole 64-bit words
    if (h_tot) std::memcpy(smp.data(), at<char>(hin, A.sample), 12 * h_tot);
    printf(" sum_desc %llu sum_p %llu sum_gate %llu sum_sample %llu", checksum(desc, sizeof(RansacDesc) * n), checksum(at<char>(hin, A.p), 48 * n_tot),
           checksum(at<char>(hin, A.gate), 16 * n_tot), checksum(smp.data(), 4 * smp.size()));
    // what came back: problem k has a hit (hypothesis 0) when k is even and it has hypotheses, best_hyp = n_hyp - 1 when k % 3 == 0;
    // pair i is flagged when i is odd, hypothesis j counted j
    void* hout = H.get<char>(A.download_bytes(want));
    RansacOut* res = at<RansacOut>(hout, A.L.in_back(A.out));
    unsigned char* flag = at<unsigned char>(hout, A.L.in_back(A.flag));
    int32_t* cnt = at<int32_t>(hout, A.L.in_back(A.cnt));   // read by unpack only when `want`
    for (int k = 0; k < n; k++) {
        std::memset(&res[k], 0, sizeof res[k]);
        const bool hyp = desc[k].n_hyp > 0;
        res[k].hit = (hyp && k % 2 == 0) ? 0 : -1;
        res[k].best_hyp = (hyp && k % 3 == 0) ? desc[k].n_hyp - 1 : -1;
        res[k].its_done = k; res[k].n_inliers = 2 * k; res[k].best_inliers = 3 * k + 1;
        for (int q = 0; q < 8; q++) { res[k].S[q] = k + q; res[k].best_S[q] = 100 + k + q; }
    }
    for (size_t i = 0; i < n_tot; i++) flag[i] = i & 1;
    for (size_t i = 0; i < h_tot && want; i++) cnt[i] = (int32_t)i;
    unsigned long long s_its = 0, s_best = 0, s_flag = 0, s_cnt = 0, s_keep = 0;
    double s_S = 0, s_bS = 0;
    for (int k = 0; k < n; k++) {
        const double before = P[k].best_S12[0];
        unpack_sim3_ransac(pp[k], rr[k], desc[k], res[k], flag, cnt);
        s_its += R[k].its_done; s_best += P[k].best_inliers; s_S += R[k].S12[7]; s_bS += P[k].best_S12[7];
        if (res[k].best_hyp < 0 && P[k].best_S12[0] == before) s_keep++;
        for (size_t i = 0; i < len[k] && (size_t)P[k].n_pairs == len[k]; i++) s_flag += R[k].inlier[i];
        for (size_t j = 0; j < hlen[k] && R[k].hyp_inliers; j++) s_cnt += R[k].hyp_inliers[j];
    }
    printf(" got_its %llu got_best %llu got_S7 %.0f got_bestS7 %.0f got_flag %llu got_cnt %llu got_keep %llu\n", s_its, s_best, s_S, s_bS, s_flag, s_cnt, s_keep);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("error load\n"); continue; }
        ransac_file(f);
        fclose(f);
    }
    return 0;
}
