// Sanitizer harness of the host half of vba_triangulate (mc_slam_amd/csrc/vba_host_triangulate.h, vba_host_arena.h): plain C++,
// built by tests/test_host_triangulate.py with g++ -fsanitize=address,undefined.
//   host_triangulate_check <file>...     one line per file: "ok key value ..." or "error <message>"
// check, describe and pack run as the driver runs them -- above 256 pairs on several threads, as small_pack_threads does -- into
// malloc'ed blocks of exactly upload_bytes(); unpack reads a block of exactly back_bytes() and writes result arrays of exactly the
// caller's sizes, so any overrun is an ASan report.  Every array of the callers is a heap block of its exact size, too.
// Checksums: sum of (2 i + 1) * word i over the 64-bit words of a region's payload (padded with zeros to whole words), mod 2^64.
// Files (little-endian, written by the test): i32 n, then per pair i32 n_matches len n_levels1 lv1 n_levels2 lv2 nulls,
// f64 c[41] (Rcw1 tcw1 Ow1 K1 Rcw2 tcw2 Ow2 K2 ratio_factor cos_max chi2_th), f64 sigma2_1[lv1] scale_1[lv1] sigma2_2[lv2]
// scale_2[lv2], f64 uv1[len][2] uv2[len][2], u8 oct1[len] oct2[len].  n_matches / n_levels are the fields, len / lv the arrays;
// nulls: 1 uv2 = NULL, 2 reason = NULL, 4 the problem itself is NULL, 8 scale_2 = NULL, 16 the result is NULL, 32 x3d = NULL
#include "../mc_slam_amd/csrc/vba_host_triangulate.h"

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
    std::vector<unsigned long long> w((bytes + 7) / 8, 0);
    if (bytes) std::memcpy(w.data(), p, bytes);
    unsigned long long s = 0;
    for (size_t i = 0; i < w.size(); i++) s += (2 * i + 1) * w[i];
    return s;
}

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
    size_t n_tot = 0, l_tot = 0, n_blocks = 0;
    std::string err;
    if (check_triangulate(n, pp.data(), rr.data(), n_tot, l_tot, n_blocks, err)) { printf("error %s\n", err.c_str()); return; }
    const TriArena A(n, n_tot, l_tot, n_blocks);
    void* hin = H.get<char>(A.L.upload_bytes());
    TriDesc* desc = at<TriDesc>(hin, A.desc);
    TriBlock* blk = at<TriBlock>(hin, A.blk);
    describe_triangulate(n, pp.data(), desc, blk);
    auto pack = [&](int k) { pack_triangulate(pp[k], desc[k], at<double>(hin, A.lev), at<double>(hin, A.uv), at<unsigned char>(hin, A.oct)); };
    if (n >= 256) {   // the threaded path: pair k goes to thread k mod 4
        std::vector<std::thread> th;
        for (int t = 0; t < 4; t++) th.emplace_back([&, t] { for (int k = t; k < n; k += 4) pack(k); });
        for (auto& t : th) t.join();
    } else
        for (int k = 0; k < n; k++) pack(k);
    printf("ok n_tot %zu l_tot %zu n_blocks %zu upload %zu back %zu total %zu desc %zu blk %zu lev %zu uv %zu oct %zu x3d %zu reason %zu", n_tot, l_tot,
           n_blocks, A.L.upload_bytes(), A.L.back_bytes(), A.L.total_bytes(), A.desc, A.blk, A.lev, A.uv, A.oct, A.x3d, A.reason);
    printf(" sum_desc %llu sum_blk %llu sum_lev %llu sum_uv %llu sum_oct %llu", checksum(desc, sizeof(TriDesc) * n), checksum(blk, sizeof(TriBlock) * n_blocks),
           checksum(at<char>(hin, A.lev), 8 * l_tot), checksum(at<char>(hin, A.uv), 32 * n_tot), checksum(at<char>(hin, A.oct), 2 * n_tot));
    // what came back: double j of the x3d region is j, match i of the call has reason i mod 9
    void* hout = H.get<char>(A.L.back_bytes());
    double* x3d = at<double>(hout, A.L.in_back(A.x3d));
    unsigned char* reason = at<unsigned char>(hout, A.L.in_back(A.reason));
    for (size_t j = 0; j < 3 * n_tot; j++) x3d[j] = (double)j;
    for (size_t i = 0; i < n_tot; i++) reason[i] = (unsigned char)(i % 9);
    long long s_acc = 0, s_status = 0, s_reason = 0;
    double s_x = 0;
    for (int k = 0; k < n; k++) {
        unpack_triangulate(rr[k], desc[k], x3d, reason);
        s_acc += R[k].n_accepted * (long long)(k + 1);
        s_status += R[k].status;
        for (size_t i = 0; i < len[k] && (size_t)P[k].n_matches == len[k]; i++) { s_reason += R[k].reason[i]; s_x += R[k].x3d[3 * i] + R[k].x3d[3 * i + 1] + R[k].x3d[3 * i + 2]; }
    }
    printf(" got_acc %lld got_status %lld got_reason %lld got_x %.0f\n", s_acc, s_status, s_reason, s_x);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("error load\n"); continue; }
        tri_file(f);
        fclose(f);
    }
    return 0;
}
