// vba_host_handle.h -- host side of the library, part 1: the handle, its device buffers and pinned staging, the copy helpers of
// an upload, the host thread pool.  Like the kernel headers, part of the one translation unit vislam_ba.hip.
#pragma once
#include "vba_host_arena.h"
#include "vba_host_layout.h"
#include "vba_host_plan.h"

#include <sched.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <atomic>
#include <memory>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    void* view = nullptr;     // small batches: the array lives inside the upload arena (one H2D for all of them); not owned
    size_t view_bytes = 0;
    void* ptr() const { return view ? view : p; }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct PinnedBuf {   // persistent pinned host staging (grown on demand)
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The arena of a small-problem entry point (vba_host_arena.h, vba_host_small.h): the device block and its pinned staging, one H2D
// of `in` and one D2H into `out` per call.  One per entry point: a call finds only its own stale bytes.
struct SideArena {
    DevBuf dev;
    PinnedBuf in, out;
    // download_bytes: what the call copies back, when that is a prefix of the back section
    hipError_t ensure(const vba_host::ArenaLayout& L, size_t download_bytes) {
        hipError_t e = dev.ensure(L.total_bytes());
        if (e == hipSuccess) e = in.ensure(L.upload_bytes());
        if (e == hipSuccess) e = out.ensure(download_bytes);
        return e;
    }
    hipError_t ensure(const vba_host::ArenaLayout& L) { return ensure(L, L.back_bytes()); }
    void release() { dev.release(); in.release(); out.release(); }
};
// vba_preintegrate (dev only), vba_pose_optimize, vba_sim3_optimize, vba_sim3_ransac, vba_triangulate, vba_two_view_init,
// vba_search_triangulation, vba_fuse, vba_posegraph_optimize, vba_search_by_sim3, vba_search_by_projection, vba_search_by_bow,
// vba_search_by_projection_kf, vba_search_for_initialization, vba_mappoint_update
enum Side { SIDE_PREINT, SIDE_POSE, SIDE_SIM3, SIDE_RANSAC, SIDE_TRI, SIDE_TWO_VIEW, SIDE_SEARCH_TRI, SIDE_FUSE, SIDE_POSEGRAPH, SIDE_SEARCH_SIM3, SIDE_SEARCH_PROJ, SIDE_SEARCH_BOW, SIDE_SEARCH_PROJ_KF, SIDE_SEARCH_INIT, SIDE_MAPPOINT, SIDE_N };

// Growable array in pinned host memory with the few std::vector members the upload / download code uses.  The staging
// arrays of a handle persist from call to call, so the H2D / D2H copies are true DMA transfers (no pageable bounce
// buffer) and run concurrently with the kernels of other streams; growth (rare after the first call) re-allocates.
template <typename T>
struct PinVec {
    typedef T value_type;
    T* p = nullptr;
    size_t n = 0, cap = 0;
    bool ok = true;   // false after a failed allocation (checked once per upload / download)
    void reserve(size_t want) {
        if (want <= cap) return;
        const size_t nc = want + want / 4 + 1024;
        void* q = nullptr;
        if (hipHostMalloc(&q, nc * sizeof(T), hipHostMallocDefault) != hipSuccess) { ok = false; return; }
        if (n) memcpy(q, p, n * sizeof(T));
        if (p) (void)hipHostFree(p);
        p = reinterpret_cast<T*>(q);
        cap = nc;
    }
    void resize(size_t m) {
        reserve(m);
        if (m <= cap) n = m;
    }
    void clear() { n = 0; }
    T* data() { return p; }
    const T* data() const { return p; }
    T& operator[](size_t i) { return p[i]; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = cap = 0;
    }
};

// pinned staging of vba_batch_upload (the concatenated arrays of a batch) and vba_batch_download
struct Staging {
    PinVec<double> pose, vel, bias, pt, uv, ow, meas, info;
    PinVec<unsigned char> kffix;
    PinVec<int> ptref, ptobs, obskf, imui, imuj, pair_a, pair_b, pimu_begin, pimu;
    PinVec<int> offpair, pairmask;
    PinVec<unsigned long long> lmask;
    PinVec<int> s_int[14];       // pinned copies of the small host-built lists (tile lists, k_lin2 runs, reference-run lists)
    PinVec<WinDesc> s_desc;
    PinVec<double> dl_pose, dl_vel, dl_bias, dl_pt, dl_chi2;
    PinVec<unsigned char> dl_outl;
    template <typename F> void each(F f) {
        f(pose); f(vel); f(bias); f(pt); f(uv); f(ow); f(meas); f(info); f(kffix);
        f(ptref); f(ptobs); f(obskf); f(imui); f(imuj); f(pair_a); f(pair_b); f(pimu_begin); f(pimu);
        f(offpair); f(pairmask); f(lmask); f(s_desc);
        for (auto& v : s_int) f(v);
        f(dl_pose); f(dl_vel); f(dl_bias); f(dl_pt); f(dl_chi2); f(dl_outl);
    }
    bool ok() { bool r = true; each([&](auto& v) { r = r && v.ok; }); return r; }
    void release() { each([](auto& v) { v.release(); }); }
};

// every device buffer of a handle, listed once: BUF_<ID>, and "<ID>" for vba_debug_buf_id (tests and scripts resolve ids by name)
#define VBA_BUFFERS(X) \
    X(DESC) X(CTRL) X(POSE) X(VEL) X(BIAS) X(KFR) X(POSE0) X(VEL0) X(BIAS0) X(POSEBK) X(VELBK) X(BIASBK) X(PT) X(PT0) X(PTBK) \
    X(PTREF) X(PTOBS) X(OBSKF) X(OBSPT) X(OBSUV) X(OBSW) X(LVL) X(CHI2E) X(CHI2F) X(DEPTH) X(EREC) X(PREC) X(SLOT) X(IMUI) \
    X(IMUJ) X(IMUMEAS) X(IMUINFO) X(IMUH) X(IMUCHI) X(S) X(LF) X(YV) X(TLSTEP) X(TLPAIR) X(TLPANB) X(TLPAN) X(VEC) X(BPOSE) \
    X(VARACT) X(PAIRA) X(PAIRB) X(ITEMBEG) X(ITEMS) X(PIMUBEG) X(PIMU) X(PART) X(OUTL) X(OUTCHI) X(LINBLK) X(OFFPAIR) \
    X(PAIRMASK) X(DBG) X(CU) X(KFFIX) X(TLKB) X(TLK) X(DVEC) X(WINV) X(SLOTPERM) X(PTPERM) X(LMASK) X(KFSEG) X(REFSEG) \
    X(ITEMMID) X(STKEY) X(LMORDER) X(SLOTOBS) X(PTINV) X(KEYSEG) X(TSLOT) X(ADJBEG) X(ADJ) X(PCGV) X(PCGM) X(KFDIR) X(MASKQ) \
    X(SLOTMASK) X(REFQ) X(PCGS) X(IMUJREC) X(ALIVE) X(SLOTO) X(SLOTREF) X(SLOTQ) X(RECQ) X(TSQ) X(RECCNT) X(RESULTS) X(PRUN0) \
    X(PREFBEG) X(PREFLIST) X(CHAINTAB) X(LMSD) X(OBSUVK)
#define VBA_BUF_ENUM(id) BUF_##id,
enum { VBA_BUFFERS(VBA_BUF_ENUM) BUF_N };
#undef VBA_BUF_ENUM

// every kernel launch of a handle is counted (vba_profile.kernel_launches: launches the last run enqueued)
#define VBA_LAUNCH(...) do { h->n_launch++; hipLaunchKernelGGL(__VA_ARGS__); } while (0)

struct ProfEvt {
    int cls;
    hipEvent_t a, b;
    int counts = 1;   // 0: the time goes to the class, but the scope is no pass of its own (the redo launches of a linearisation pass)
};

// Host threads that the stages of asynchronous batches (vba_batch_submit) share: the packing of one ticket may run while another
// ticket's results are scattered.  A pool takes what is free when it starts (at least one thread: it waits for it) and gives it
// back when it ends, so the stages together never use more than vba_host_threads().
struct HostBudget {
    std::mutex mu;
    std::condition_variable cv;
    int free = 0;
    int take(int want) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return free > 0; });
        const int t = std::max(1, std::min(want, free));
        free -= t;
        return t;
    }
    void give(int t) {
        {
            std::lock_guard<std::mutex> lk(mu);
            free += t;
        }
        cv.notify_all();
    }
};
struct AsyncState;   // the tickets, arenas and workers of vba_batch_submit (defined with it)

struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<hipStream_t> xstreams;  // extra streams: one per window group of a large batch
    // upload (H2D + structure build) and download (D2H) streams: the run stream itself, except for the lanes of
    // vba_batch_solve, which share the parent's four streams -- run x 2, upload, download -- one per hardware queue
    hipStream_t up_stream = nullptr, dl_stream = nullptr;
    bool owns_streams = true;
    std::string err;
    DevBuf buf[BUF_N];
    SideArena side[SIDE_N];       // one per small-problem entry point
    // small batches (UploadPlan::arena_on): every host-built array of an upload goes through ONE pinned arena and ONE H2D copy
    struct Pending { int id; const void* src; size_t bytes; };
    std::vector<Pending> pending;
    DevBuf up_arena;
    PinnedBuf up_arena_host;
    Staging stg;   // pinned staging: upload arrays; download: one D2H per array, windows scattered to the callers' arrays by host threads
    std::vector<Handle*> lanes;   // sub-handles of vba_batch_solve (chunks of a large batch in flight concurrently)
    bool is_lane = false;
    AsyncState* as = nullptr;     // vba_batch_submit: created at the first submit (its arenas are lanes too, kept apart from `lanes`)
    int async_depth = 2;          // vba_batch_set_depth: batches resident on the device at once
    HostBudget* budget = nullptr; // an arena of vba_batch_submit: its packing and scatter pools draw threads from the parent's budget
    bool hip_failed = false;      // a HIP call of this handle failed (HIPCHK): tells a device error from a rejected window
    Batch B;
    std::vector<WinDesc> desc;
    PinVec<WinCtrl> hctrl;    // the control blocks after a run (pinned: the copy rides on the run's stream)
    std::vector<int> one_sb;      // n_win == 1: the window's step table (first pair of every factorisation step), for StepOne
    PinnedBuf res_host;           // few windows: control blocks + every result array in ONE block (device: BUF_RESULTS), one D2H copy
    size_t res_bytes = 0, res_off[7] = {0, 0, 0, 0, 0, 0, 0};   // ctrl, pose, vel, bias, pt, outlier flags, chi2
    hipEvent_t up_done = nullptr; // recorded behind an upload that was not waited for on the host (vba_solve)
    bool up_pending = false;
    bool dl_prefetched = false;   // few windows: the run left the result arrays in the download staging already
    int n_win = 0;
    vba_host::Overrides ov;   // what the vba_debug_set_* hooks set
    vba_host::UploadPlan up;  // the policy of the uploaded batch (vba_host_plan.h), fixed at upload_begin
    vba_host::RunPlan rp;     // ... and of the run being enqueued / the last run
    vba_host::LaunchGeom geom;   // launch geometry (maxima over the batch)
    std::vector<int> win_tiles;  // tile products of one factorisation of window w
    std::vector<long long> win_prod_order;  // per window: tile products under the V/Bias-first and the keyframe order (-1: not evaluated)
    int algo = 0, variant = 2, solver = 0;
    volatile int* stop_host = nullptr;  // pinned, device-visible
    int* stop_dev = nullptr;
    bool profile = false;
    long long n_launch = 0;   // kernel launches enqueued through this handle so far
#ifdef VBA_TEST_HOOKS
    // vba_debug_capture: at the cap_call-th enqueue_solve_iteration of the next run, device copies of the stage products
    int cap_call = -1, cap_count = 0, cap_done = 0;
    int cap_path[4] = {-1, -1, -1, -1};   // kernels that iteration enqueued: Schur, factor, triangular solve (CAP_SCHUR_* ...)
    DevBuf cap[16];
    size_t cap_bytes[16] = {0};
#endif
    std::vector<ProfEvt> evts;
    std::vector<hipEvent_t> evt_pool;
    size_t evt_used = 0;
    vba_profile prof;
    bool uploaded = false;
    bool ran = false;
};

#define HIPCHK(h, call)                                                                          \
    do {                                                                                          \
        hipError_t _e = (call);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(_e);                         \
            (h)->hip_failed = true;                                                               \
            return -1;                                                                            \
        }                                                                                         \
    } while (0)

int fail(Handle* h, const std::string& m) {
    static std::mutex mu;   // build_structure runs on several host threads during an upload
    std::lock_guard<std::mutex> lk(mu);
    h->err = m;
    return -1;
}

template <typename T>
T* dp(Handle* h, int id) {
    return reinterpret_cast<T*>(h->buf[id].ptr());
}

hipEvent_t get_evt(Handle* h) {
    if (h->evt_used == h->evt_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        h->evt_pool.push_back(e);
    }
    return h->evt_pool[h->evt_used++];
}

struct ProfScope {
    Handle* h;
    hipStream_t stream;
    ProfEvt e;
    bool on;
    ProfScope(Handle* hh, hipStream_t st, int cls) : h(hh), stream(st), on(hh->profile) {
        if (on) {
            e.cls = cls;
            e.a = get_evt(h);
            e.b = get_evt(h);
            (void)hipEventRecord(e.a, stream);
        }
    }
    ~ProfScope() {
        if (on) {
            (void)hipEventRecord(e.b, stream);
            h->evts.push_back(e);
        }
    }
};

// ---- structure build, host half: csrc/vba_host_structure.h (plain C++, also compiled into the sanitizer harness of the tests)
using vba_host::Structure;
using vba_host::vpos_host;
using vba_host::now_ms;
using vba_host::quat_to_R_host;
using vba_host::LaunchGeom;
int build_structure(Handle* h, const vba_problem* P, Structure& st, bool two_sided = false) {
    std::string err;
    if (vba_host::build_structure(P, st, err, two_sided)) return fail(h, err);
    if (h->ov.path.lin_fallback && P->variant != VBA_VARIANT_PRV_IDP) st.linblk.clear();   // test hook: the thread-per-landmark linearisation
    return 0;
}

// a pageable std::vector goes through a pinned copy first: a pageable hipMemcpyAsync is a synchronous, staged transfer
template <typename T>
int h2d_vec(Handle* h, int id, const std::vector<T>& v, PinVec<T>& pin) {
    if (h->up.arena_on) {
        h->pending.push_back({id, v.data(), v.size() * sizeof(T)});
        return 0;
    }
    pin.clear();
    pin.resize(v.size());
    if (!pin.ok) return fail(h, "out of pinned host memory (upload staging)");
    if (!v.empty()) memcpy(pin.data(), v.data(), v.size() * sizeof(T));
    HIPCHK(h, h->buf[id].ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) HIPCHK(h, hipMemcpyAsync(h->buf[id].p, pin.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->up_stream));
    return 0;
}

template <typename V>
int h2d(Handle* h, int id, const V& v) {
    typedef typename V::value_type T;
    if (h->up.arena_on) {
        h->pending.push_back({id, v.data(), v.size() * sizeof(T)});
        return 0;
    }
    HIPCHK(h, h->buf[id].ensure(std::max<size_t>(v.size() * sizeof(T), 16)));
    if (!v.empty()) HIPCHK(h, hipMemcpyAsync(h->buf[id].p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->up_stream));
    return 0;
}
// arena mode: lay the recorded arrays out (256-B aligned), gather them into the pinned arena, one copy, point the views
int h2d_flush(Handle* h) {
    if (!h->up.arena_on) return 0;
    size_t total = 0;
    for (auto& q : h->pending) total += (std::max<size_t>(q.bytes, 16) + 255) / 256 * 256;
    HIPCHK(h, h->up_arena.ensure(total + 256));
    HIPCHK(h, h->up_arena_host.ensure(total + 256));
    char* hb = reinterpret_cast<char*>(h->up_arena_host.p);
    char* db = reinterpret_cast<char*>(h->up_arena.p);
    size_t off = 0;
    for (auto& q : h->pending) {
        if (q.bytes) memcpy(hb + off, q.src, q.bytes);
        h->buf[q.id].view = db + off;
        h->buf[q.id].view_bytes = std::max<size_t>(q.bytes, 16);
        off += (std::max<size_t>(q.bytes, 16) + 255) / 256 * 256;
    }
    if (total) HIPCHK(h, hipMemcpyAsync(db, hb, total, hipMemcpyHostToDevice, h->up_stream));
    h->pending.clear();
    return 0;
}
int dalloc(Handle* h, int id, size_t bytes) {
    HIPCHK(h, h->buf[id].ensure(std::max<size_t>(bytes, 16)));
    return 0;
}

// Host threads of one handle (packing, structure build, scatter).  One process per GPU: the ranks of a node share its cores, so
// the pool is this rank's share -- cores / LOCAL_WORLD_SIZE, at most 16, at least 2 -- unless VBA_UPLOAD_THREADS says otherwise
// (mc_slam_amd/launch.py exports it per rank).  The cores are those the process may run on (sched_getaffinity: a rank pinned to its
// share by the launcher counts only that share).
int host_threads() {
    static const int n = [] {
        const vba_host::Knobs& K = vba_host::process_knobs();
        if (K.upload_threads != vba_host::KNOB_UNSET) return std::max(1, K.upload_threads);
        int cores = (int)std::thread::hardware_concurrency();
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof set, &set) == 0 && CPU_COUNT(&set) > 0) cores = CPU_COUNT(&set);
        // ranks of THIS node that share the cores (torchrun exports LOCAL_WORLD_SIZE; WORLD_SIZE counts the ranks of other nodes too
        // and is not used).  A rank counts as pinned to its share only when the launcher says so (mc_slam_amd/launch.py exports
        // VBA_RANK_CPUS with the cores it bound the rank to): a cpuset-limited container also shows fewer cores than the machine
        // has, and there the ranks still share what it shows.
        const int share = K.rank_cpus ? cores : std::max(1, cores / std::max(1, K.local_world_size));
        return std::max(std::min(2, std::max(1, cores)), std::min(16, share));
    }();
    return n;
}
// job(0) .. job(count - 1) on up to want_threads host threads (this one included), dealt out one index at a time; an arena of
// vba_batch_submit takes its threads from the parent's budget
template <typename F>
void host_parallel_for(Handle* h, int count, int want_threads, const F& job) {
    std::atomic<int> next(0);
    auto work = [&]() {
        for (int q = next.fetch_add(1); q < count; q = next.fetch_add(1)) job(q);
    };
    const int nt = h->budget ? h->budget->take(want_threads) : want_threads;
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    if (h->budget) h->budget->give(nt);
}
}  // namespace
