// vislam_ba.hip -- C-ABI (include/vislam_ba.h) of the MI355X local-BA backend, one translation unit: the kernel headers, the host
// side by topic, and below the extern "C" entry points.
//   the solve     vba_host_structure.h (plain-C++ structure build), vba_host_handle.h (handle and buffers), vba_host_upload.h (H2D +
//                 structure build), vba_host_run.h (the lock-step launch schedule of the two-stage solve and the download),
//                 vba_host_batch.h (lanes and tickets): vba_create / destroy / last_error, vba_solve*, vba_batch_upload / run /
//                 download / solve*, vba_batch_set_depth / submit* / poll / wait
//   small problems  vba_host_small.h: one driver over the plain-C++ call object of each topic (vba_host_<topic>.h).  Tracking:
//                 vba_preintegrate, vba_search_by_projection and vba_search_by_bow (the matchers in front of) vba_pose_optimize.  Initialisation: vba_search_for_initialization (the matcher in front of) vba_two_view_init.  Local mapping:
//                 vba_search_triangulation (the matcher in front of) vba_triangulate, vba_fuse, vba_mappoint_update (what refreshes the points between them and the BA).  Loop closing: vba_search_by_bow, vba_sim3_ransac,
//                 vba_search_by_sim3, vba_sim3_optimize, vba_search_by_projection_kf (the matcher behind it), vba_posegraph_optimize.
//                 Relocalisation: vba_search_by_bow, vba_search_by_projection_kf between two vba_pose_optimize calls
//   the rest      vba_host_hooks.h (vba_debug_*, hooks flavour), vba_host_threads, vba_set_profile / get_profile
//
// Host-side control flow restated from src/Optimizer.cpp:453-517 (two-stage protocol) and
// Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:354-419 (optimize loop); all per-iteration decisions are taken
// on the device (k_ctrl_*), the host only enqueues.  No CPU fallback exists: without a HIP device every entry
// point fails with an error.
#include "../../include/vislam_ba.h"
#include "vba_host_structure.h"
#include "vba_host_posegraph.h"
#include "vba_problem_io.h"
#include "vba_kernels_lm.h"
#include "vba_preint.h"
#include "vba_pose.h"
#include "vba_sim3.h"
#include "vba_sim3_ransac.h"
#include "vba_triangulate.h"
#include "vba_two_view.h"
#include "vba_search_tri.h"
#include "vba_fuse.h"
#include "vba_search_sim3.h"
#include "vba_search_proj.h"
#include "vba_search_proj_kf.h"
#include "vba_search_bow.h"
#include "vba_search_init.h"
#include "vba_mappoint.h"
#include "vba_posegraph.h"
#include "vba_structure.h"
#include "vba_pcg.h"
#include "vba_chain.h"

#include "vba_host_handle.h"
#include "vba_host_upload.h"
#include "vba_host_run.h"
#include "vba_host_batch.h"
#include "vba_host_small.h"
#include "vba_host_hooks.h"

namespace {
// the handle of an entry point that needs it idle; nullptr (the entry point returns -1) for no handle or one with tickets in flight
Handle* idle_handle(void* handle) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    return (h && !async_busy(h)) ? h : nullptr;
}
}  // namespace

extern "C" {

int vba_create(int device, void** handle) {
    if (!handle) return -1;
    *handle = nullptr;
    Handle* h = nullptr;
    const int rc = make_handle(device, nullptr, &h);
    if (rc == 0) *handle = h;
    return rc;
}

int vba_destroy(void* handle) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    if (h->as) async_shutdown(h);
    for (Handle* l : h->lanes) (void)vba_destroy(l);
    h->lanes.clear();
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(h->up_stream);
    (void)hipStreamSynchronize(h->dl_stream);
    h->stg.release();
    h->hctrl.release();
    h->res_host.release();
    h->up_arena.release();
    h->up_arena_host.release();
    for (auto& b : h->buf) b.release();
#ifdef VBA_TEST_HOOKS
    for (auto& b : h->cap) b.release();
#endif
    for (auto& a : h->side) a.release();
    for (auto e : h->evt_pool) (void)hipEventDestroy(e);
    if (h->up_done) (void)hipEventDestroy(h->up_done);
    if (h->owns_streams)
        for (auto st : h->xstreams) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (h->stop_host) (void)hipHostFree((void*)h->stop_host);
    if (h->owns_streams) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

const char* vba_last_error(void* handle) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    return h ? h->err.c_str() : "null handle";
}

int vba_batch_upload(void* handle, int32_t n, vba_problem* const* problems) {
    Handle* h = idle_handle(handle);
    return h ? do_upload(h, n, problems) : -1;
}
int vba_batch_run(void* handle, const volatile int* stop_flag) {
    Handle* h = idle_handle(handle);
    return h ? do_run(h, stop_int(stop_flag)) : -1;
}
int vba_batch_run_b(void* handle, const volatile unsigned char* stop_flag) {
    Handle* h = idle_handle(handle);
    return h ? do_run(h, stop_byte(stop_flag)) : -1;
}
int vba_batch_download(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? do_download(h, n, inout, out) : -1;
}
int vba_solve(void* handle, vba_problem* inout, vba_result* out, const volatile int* stop_flag) { return solve_one(handle, inout, out, stop_int(stop_flag)); }
int vba_solve_b(void* handle, vba_problem* inout, vba_result* out, const volatile unsigned char* stop_flag) { return solve_one(handle, inout, out, stop_byte(stop_flag)); }
int vba_batch_solve(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out, const volatile int* stop_flag) {
    return batch_solve(handle, n, inout, out, stop_int(stop_flag));
}
int vba_batch_solve_b(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out, const volatile unsigned char* stop_flag) {
    return batch_solve(handle, n, inout, out, stop_byte(stop_flag));
}

int vba_batch_set_depth(void* handle, int32_t depth) {
    Handle* h = idle_handle(handle);
    if (!h) return -1;
    if (depth < 1 || depth > 4) return fail(h, "vba_batch_set_depth: depth must be 1..4");
    if (h->as) {   // idle: the workers leave, arenas beyond the new depth free their device buffers and staging
        AsyncState& A = *h->as;
        async_stop_workers(A);
        while ((int)A.arenas.size() > depth) {
            (void)vba_destroy(A.arenas.back());
            A.arenas.pop_back();
        }
    }
    h->async_depth = depth;
    return 0;
}
int vba_batch_submit(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out, const volatile int* stop_flag,
                     int64_t* ticket) {
    return submit(reinterpret_cast<Handle*>(handle), n, inout, out, stop_int(stop_flag), ticket);
}
int vba_batch_submit_b(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out,
                       const volatile unsigned char* stop_flag, int64_t* ticket) {
    return submit(reinterpret_cast<Handle*>(handle), n, inout, out, stop_byte(stop_flag), ticket);
}
int vba_batch_poll(void* handle, int64_t ticket) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    if (!h->as || !h->as->tickets.count(ticket)) return fail(h, "vba_batch_poll: unknown or retired ticket " + std::to_string(ticket));
    AsyncState& A = *h->as;
    std::lock_guard<std::mutex> lk(A.mu);
    return A.tickets[ticket]->done ? 0 : 1;
}
int vba_batch_wait(void* handle, int64_t ticket) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    if (!h->as || !h->as->tickets.count(ticket)) return fail(h, "vba_batch_wait: unknown or retired ticket " + std::to_string(ticket));
    AsyncState& A = *h->as;
    std::shared_ptr<AsyncTicket> t = A.tickets[ticket];
    {
        std::unique_lock<std::mutex> lk(A.mu);
        A.cv.wait(lk, [&] { return t->done; });
    }
    A.tickets.erase(ticket);
    if (t->rc)
        return fail(h, "vba_batch_submit, ticket " + std::to_string(ticket) + ", windows 0.." + std::to_string(t->inout.size() - 1) + ": " + t->err);
    return 0;
}

// the size of the host thread pool of a handle in this process (this rank's share of the cores: host_threads above)
int vba_host_threads(void) { return host_threads(); }

// ---- the small-problem entry points: a handle check and one call (the drivers: vba_host_small.h)
int vba_preintegrate(void* handle, int32_t n_edges, const int32_t* sample_begin, const double* gyr, const double* acc,
                     const double* dt, double gyr_meas_cov, double acc_meas_cov, double* imu_meas, double* cov_pvphi,
                     double* imu_info_prv) {
    Handle* h = idle_handle(handle);
    return h ? preintegrate(h, n_edges, sample_begin, gyr, acc, dt, gyr_meas_cov, acc_meas_cov, imu_meas, cov_pvphi, imu_info_prv) : -1;
}
int vba_pose_optimize(void* handle, int32_t n_frames, vba_frame_problem* const* inout, vba_frame_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? pose_optimize(h, n_frames, inout, out) : -1;
}
int vba_sim3_optimize(void* handle, int32_t n_problems, vba_sim3_problem* const* inout, vba_sim3_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? sim3_optimize(h, n_problems, inout, out) : -1;
}
int vba_sim3_ransac(void* handle, int32_t n_problems, vba_sim3_ransac_problem* const* inout, vba_sim3_ransac_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? sim3_ransac(h, n_problems, inout, out) : -1;
}
int vba_triangulate(void* handle, int32_t n_pairs, vba_triangulate_problem* const* in, vba_triangulate_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? triangulate(h, n_pairs, in, out) : -1;
}
int vba_two_view_init(void* handle, int32_t n_problems, vba_two_view_problem* const* in, vba_two_view_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? two_view_init(h, n_problems, in, out) : -1;
}
int vba_search_triangulation(void* handle, int32_t n_pairs, vba_search_tri_problem* const* in, vba_search_tri_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? search_triangulation(h, n_pairs, in, out) : -1;
}
int vba_fuse(void* handle, int32_t n_problems, vba_fuse_problem* const* in, vba_fuse_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? fuse(h, n_problems, in, out) : -1;
}
int vba_search_by_sim3(void* handle, int32_t n_pairs, vba_search_sim3_problem* const* in, vba_search_sim3_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? search_by_sim3(h, n_pairs, in, out) : -1;
}
int vba_search_by_projection(void* handle, int32_t n_problems, vba_search_proj_problem* const* in, vba_search_proj_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? search_by_projection(h, n_problems, in, out) : -1;
}
int vba_search_by_projection_kf(void* handle, int32_t n_problems, vba_search_proj_kf_problem* const* in, vba_search_proj_kf_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? search_by_projection_kf(h, n_problems, in, out) : -1;
}
int vba_search_by_bow(void* handle, int32_t n_pairs, vba_search_bow_problem* const* in, vba_search_bow_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? search_by_bow(h, n_pairs, in, out) : -1;
}
int vba_search_for_initialization(void* handle, int32_t n_pairs, vba_search_init_problem* const* in, vba_search_init_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? search_for_initialization(h, n_pairs, in, out) : -1;
}
int vba_mappoint_update(void* handle, int32_t n_problems, vba_mappoint_problem* const* in, vba_mappoint_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? mappoint_update(h, n_problems, in, out) : -1;
}
int vba_posegraph_optimize(void* handle, int32_t n_graphs, vba_posegraph_problem* const* inout, vba_posegraph_result* const* out) {
    Handle* h = idle_handle(handle);
    return h ? posegraph_run(h, n_graphs, inout, out, nullptr) : -1;
}

#ifdef VBA_TEST_HOOKS
// test hook (not part of include/vislam_ba.h): H (dense, [7 n_free]^2 row-major), b and the x of the first trial of the first
// iteration of one graph, as k_posegraph_opt formed them; the graph's arrays are left untouched
int vba_debug_posegraph_system(void* handle, vba_posegraph_problem* graph, double* H, double* b, double* x) {
    Handle* h = idle_handle(handle);
    if (!h) return -1;
    if (!graph || !H || !b || !x) return fail(h, "vba_debug_posegraph_system: bad arguments");
    PgDebug dbg{H, b, x};
    vba_posegraph_result r;
    vba_posegraph_result* rp = &r;
    return posegraph_run(h, 1, &graph, &rp, &dbg);
}
#endif

int vba_set_profile(void* handle, int32_t enable) {
    Handle* h = idle_handle(handle);
    if (!h) return -1;
    h->profile = enable != 0;
    return 0;
}
int vba_get_profile(void* handle, vba_profile* out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !out) return -1;
    *out = h->prof;
    return 0;
}

}  // extern "C"
