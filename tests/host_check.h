// What the sanitizer harnesses tests/host_*_check.cpp share (plain C++, built by tests/host_check_lib.py with g++
// -fsanitize=address,undefined): exact-size heap blocks, the checksum of a packed region, the loop over the files of the command
// line, and run_call, which drives the call object of a small-problem entry point (mc_slam_amd/csrc/vba_host_<topic>.h) through the
// host sequence of the library's driver (run_small, vba_host_small.h).
#pragma once
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

struct Heap {   // exact-size heap blocks, freed at the end of a file
    std::vector<void*> all;
    template <class T> T* get(size_t n) { void* p = malloc(n * sizeof(T) + (n == 0)); all.push_back(p); return static_cast<T*>(p); }
    template <class T> T* fill(size_t n, T v) { T* p = get<T>(n); for (size_t i = 0; i < n; i++) p[i] = v; return p; }
    template <class T> T* read(FILE* f, size_t n, bool& ok) { T* p = get<T>(n); ok = ok && (n == 0 || fread(p, sizeof(T), n, f) == n); return p; }
    ~Heap() { for (void* p : all) free(p); }
};

// sum of (2 i + 1) * word i over the 64-bit words of a region's payload (padded with zeros to whole words), mod 2^64.  pos: the
// region continues a payload of *pos words (and *pos moves on)
inline unsigned long long checksum(const void* p, size_t bytes, unsigned long long* pos = nullptr) {
    std::vector<unsigned long long> w((bytes + 7) / 8, 0);
    if (bytes) std::memcpy(w.data(), p, bytes);
    unsigned long long s = 0, i0 = pos ? *pos : 0;
    for (size_t i = 0; i < w.size(); i++) s += (2 * (i0 + i) + 1) * w[i];
    if (pos) *pos += w.size();
    return s;
}

// " bind_<field> <offset>": where a pointer of the Batch that bind(base) returned points, as a byte offset from base
#define PRINT_BIND(B, base, field) printf(" bind_" #field " %zu", (size_t)((const char*)(B).field - (const char*)(base)))

// The host sequence of run_small on heap blocks of exactly the call's sizes, so any overrun is an ASan report: prepare, describe,
// pack (from 256 problems up on four threads, problem k on thread k mod 4), bind on the staging block, packed(B, hin) to print
// "ok" and what was packed, a block of exactly download_bytes() that back(hout) fills with what "came back", unpack.  false: the
// call was refused and "error <message>" is printed
template <class Call, class P, class R, class Packed, class Back>
bool run_call(Heap& H, Call& C, int n, P* const* pp, R* const* rr, const Packed& packed, const Back& back) {
    std::string err;
    if (C.prepare(n, pp, rr, err)) { printf("error %s\n", err.c_str()); return false; }
    void* hin = H.get<char>(C.layout().upload_bytes());
    C.describe(pp, hin);
    std::atomic<const char*> refused(nullptr);
    auto pack = [&](int k) { if (const char* why = C.pack(k, pp[k], hin)) refused.store(why); };
    if (n >= 256) {
        std::vector<std::thread> th;
        for (int t = 0; t < 4; t++) th.emplace_back([&, t] { for (int k = t; k < n; k += 4) pack(k); });
        for (auto& t : th) t.join();
    } else
        for (int k = 0; k < n; k++) pack(k);
    if (const char* why = refused.load()) { printf("error %s\n", why); return false; }
    packed(C.bind(hin), hin);
    void* hout = H.get<char>(C.download_bytes());
    back(hout);
    for (int k = 0; k < n; k++) C.unpack(k, pp[k], rr[k], hin, hout);
    return true;
}

// file(f) for every file named from argv[first] on; a file that cannot be opened is a line "error load"
template <class F>
int for_each_file(int argc, char** argv, int first, const F& file) {
    for (int a = first; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("error load\n"); continue; }
        file(f);
        fclose(f);
    }
    return 0;
}
